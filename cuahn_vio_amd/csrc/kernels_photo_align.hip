// kernels_photo_align.hip — photometric alignment on the four corner offsets, in its two forms (include/hnet.h): the plain one, single level or coarse to
// fine (hnet_photo_align; photo_pyramid_dev.h), and the one with a gain / bias model and Huber weights (hnet_photo_robust; photo_robust_dev.h;
// DESIGN 7n).  Forward-additive Lucas-Kanade / Levenberg-Marquardt on the squared form of the residual kernels_photo.hip sums.  The pyramid is
// kernels_photo_pyramid.hip's.
//
// Three accumulate kernels, one linearisation into one partial per (row slice, pair) each: photo_align_accum_kernel (plain, level 0),
// photo_pyr_accum_kernel<1..3> (plain, coarse levels), photo_robust_accum_kernel<0..3>.  They share a skeleton - one workgroup of 256 / 256 / 128 / 64
// threads per (row slice, pair), the pair's level-L img2 staged in LDS with 16-byte loads, lane 0 forms H from the start or the trial point, quads of 4
// consecutive pixels at level 0 and a stride of the workgroup above, double accumulators and counts per thread, lanes reduced by the fixed __shfl_down tree,
// the waves in wave order through LDS, no floating-point atomics - and stand three times ON PURPOSE: written once as a function template over the level and
// a terms type, the records kept their bytes but every accumulate launch measured 0.4 - 1.9 us longer on an MI355X.  The per-pixel quantity of
// the coarse and the robust kernels is include/hnet_photo_pyramid.h's; at L = 0 it is, bit for bit, what photo_align_accum_kernel writes out inline (also on purpose: on those
// functions the plain calls measured 1.5 - 3 % slower).  A
// product (double) s_i * (double) s_j of two floats is exact in a double: the device and the host reference differ in the ORDER of the additions only.
// photo_align_solve_kernel / photo_robust_solve_kernel (one workgroup of 64 lanes per pair) add the 7 partials in slice order, form D, T, A and g entry by
// entry over their lanes (hnet_align::form_T / form_A / form_g, hnet_robust::form_A10 / form_g10: the host reference runs the same functions in a loop) and
// lane 0 takes the step (hnet_align::step, hnet_robust::step).  112, 56 and 28 rows divide by PHOTO_SLICES = 7, so a solve kernel serves every level.
// The solve kernels do not write the trial H as nine floats: they write the trial point and lane 0 of every accumulate workgroup forms H from it.
//
// The start of a level is where the level above ended, whatever its flags: a gather kernel copies it, as bits (a NaN keeps its payload), from the records
// into the contiguous array the accumulate and solve kernels read.  Levels and iterations are separate launches; nothing waits on another workgroup, and a
// stopped pair's workgroups return at once (a workgroup-uniform branch).  pa_run_levels is the one launch sequence of both forms, and of a third: the
// robust form on the template pixels a mask admits (MaskedForm), whose accumulate kernels and mask pyramid are kernels_photo_masked.hip's.
#include "photo_masked_dev.h"
#include "photo_robust_kernel_dev.h"

namespace hnet {

namespace pa = hnet_align;
namespace pr = hnet_robust;

// the constants and the device functions of the kernels below
namespace {
constexpr int PA_THREADS = 256, PA_WAVES = PA_THREADS / 64;
constexpr int PA_QUADS = PHOTO_SLICE_PIX / (4 * PA_THREADS);                  // 10 quads per thread
static_assert(offsetof(AlignSums, sr) == pa::NSYM * 8 && offsetof(AlignSums, rr) == (pa::NSYM + pa::NH) * 8 && offsetof(AlignSums, n_valid) == PA_ND * 8,
              "AlignSums is 55 doubles, then the count");
// dynamic LDS of the accumulate kernel: img2 | per-wave sums [4][55] f64 | per-wave counts [4] i32 | H [9] f32 | flag
constexpr int PA_LDS_BYTES = NPIX + PA_WAVES * PA_ND * 8 + PA_WAVES * 4 + 9 * 4 + 4;      // 73 496: two workgroups per CU
static_assert(NPIX % 16 == 0 && 2 * PA_LDS_BYTES <= 160 * 1024, "aligned sections; two workgroups share a CU's LDS");
constexpr int pl_threads(int L) { return L == 1 ? 256 : (L == 2 ? 128 : 64); }  // plain, levels 1 - 3: 10, 5 and 2.5 pixels per thread and slice
// (the robust kernel's threads, LDS layout and pr_pixel: photo_robust_kernel_dev.h, shared with kernels_photo_masked.hip)

// The front of both solve kernels, over the 64 lanes of the workgroup: the ND sums and the two count words of the pair's 7 partials added in slice order,
// the degenerate test of the linearisation point x, and D column by column; then a barrier.  The arrays are the calling kernel's own __shared__ arrays (an
// array that only lane 0 touches stays out of LDS that way; a member of a shared struct could not).
template <int ND, class Sums>
__device__ __forceinline__ void pa_solve_front(const Sums* part, const float* x, double* sums, int* cnt, int* degenerate, double* D) {
    const int tid = threadIdx.x;
    for (int e = tid; e < ND + 2; e += 64) {
        if (e < ND) {
            double t = 0.0;
#pragma unroll
            for (int s = 0; s < PHOTO_SLICES; s++) t += reinterpret_cast<const double*>(part + s)[e];
            sums[e] = t;
        } else {
            int t = 0;
#pragma unroll
            for (int s = 0; s < PHOTO_SLICES; s++) t += reinterpret_cast<const int*>(reinterpret_cast<const double*>(part + s) + ND)[e - ND];
            cnt[e - ND] = t;
        }
    }
    if (tid == 63) {
        float h[9];
        *degenerate = pa_homography(x, h) ? 0 : 1;
    }
    if (tid < pa::NX) {
        double dst[8], col[pa::NH];
#pragma unroll
        for (int k = 0; k < 8; k++) dst[k] = pa::corner(p4(k), x[k]);
        pa::dlt_jacobian_col(dst, tid, col);
#pragma unroll
        for (int i = 0; i < pa::NH; i++) D[i * pa::NX + tid] = col[i];
    }
    __syncthreads();
}
// T = (sum s s^T) D entry by entry; then a barrier
__device__ __forceinline__ void pa_solve_T(const double* ss, const double* D, double* T) {
    for (int e = threadIdx.x; e < pa::NH * pa::NX; e += 64) T[e] = pa::form_T(ss, D, e / pa::NX, e % pa::NX);
    __syncthreads();
}
static_assert(PHOTO_SLICES == 7, "the solve kernels add 7 partials");

}  // namespace

// grid: PHOTO_SLICES * n workgroups (slice = block % PHOTO_SLICES).  x0 != nullptr: the first linearisation, at x0 [n][8]; otherwise at work[pair].x_trial,
// and a pair whose record carries a flag has stopped: its workgroups return at once (rec was written by the solve launch before this one).
__global__ __launch_bounds__(PA_THREADS) void photo_align_accum_kernel(const uint8_t* __restrict__ img1, const uint8_t* __restrict__ img2,
                                                                       const float* __restrict__ x0, const AlignWork* __restrict__ work,
                                                                       const AlignRec* __restrict__ rec, AlignSums* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) uint8_t pa_lds[];
    const int pair = blockIdx.x / PHOTO_SLICES, slice = blockIdx.x - pair * PHOTO_SLICES;
    if (!x0 && rec[pair].flags != 0) return;                                  // (workgroup-uniform)
    double* w_sum = reinterpret_cast<double*>(pa_lds + NPIX);
    int* w_cnt = reinterpret_cast<int*>(w_sum + PA_WAVES * PA_ND);
    float* hs = reinterpret_cast<float*>(w_cnt + PA_WAVES);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {
        const uint4* src = reinterpret_cast<const uint4*>(img2 + (size_t)pair * NPIX);
        for (int i = tid; i < NPIX / 16; i += PA_THREADS) reinterpret_cast<uint4*>(pa_lds)[i] = src[i];
    }
    if (tid == 0) {
        float h[9];
        pa_homography(x0 ? x0 + (size_t)pair * 8 : work[pair].x_trial, h);
#pragma unroll
        for (int k = 0; k < 9; k++) hs[k] = h[k];
    }
    __syncthreads();
    float h[9];
#pragma unroll
    for (int k = 0; k < 9; k++) h[k] = hs[k];

    const uint8_t* tile = pa_lds;
    const uint8_t* a_img = img1 + (size_t)pair * NPIX;
    const int pix0 = slice * PHOTO_SLICE_PIX + 4 * tid;
    double acc[PA_ND];
#pragma unroll
    for (int k = 0; k < PA_ND; k++) acc[k] = 0.0;
    int n_valid = 0;
    for (int q = 0; q < PA_QUADS; q++) {
        const int pix = pix0 + q * (4 * PA_THREADS);
        const int v = pix / IMG_W, u0 = pix - v * IMG_W;
        const uint32_t a4 = *reinterpret_cast<const uint32_t*>(a_img + pix);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            float ix, iy, Z;
            warp_coords(h, u0 + j, v, ix, iy, Z);
            if (!(ix >= 0.0f && ix < (float)(IMG_W - 1) && iy >= 0.0f && iy < (float)(IMG_H - 1))) continue;      // (false for NaN)
            // the four taps: warp_taps_global's expressions, every tap inside
            const float x0f = floorf(ix), y0f = floorf(iy);
            const float wx1 = ix - x0f, wx0 = 1.0f - wx1, wy1 = iy - y0f, wy0 = 1.0f - wy1;
            const uint8_t* p = tile + (int)y0f * IMG_W + (int)x0f;
            const float a = PixRead<uint8_t>::cvt(p[0]), b = PixRead<uint8_t>::cvt(p[1]);
            const float c = PixRead<uint8_t>::cvt(p[IMG_W]), d = PixRead<uint8_t>::cvt(p[IMG_W + 1]);
            float w = fmaf(a, wx0 * wy0, 0.0f);
            w = fmaf(b, wx1 * wy0, w);
            w = fmaf(c, wx0 * wy1, w);
            w = fmaf(d, wx1 * wy1, w);
            const float r = (w - PixRead<uint8_t>::cvt((uint8_t)(a4 >> (8 * j)))) * 255.0f;
            // the gradient of the sampled function and the row of dr / dvec(H); every operation is written out (one rounding each, as the host reference)
            const float gx = fmaf(d - c, wy1, (b - a) * wy0) * 255.0f;
            const float gy = fmaf(d - b, wx1, (c - a) * wx0) * 255.0f;
            const float qq = fmaf(gx, ix, gy * iy);
            const float rz = 1.0f / Z, au = (float)(u0 + j) * rz, av = (float)v * rz;
            const float s[pa::NH] = {gx * au, gx * av, gx * rz, gy * au, gy * av, gy * rz, -qq * au, -qq * av, -qq * rz};
            double sd[pa::NH];
#pragma unroll
            for (int i = 0; i < pa::NH; i++) sd[i] = (double)s[i];
            const double rd = (double)r;
#pragma unroll
            for (int i = 0; i < pa::NH; i++) {
#pragma unroll
                for (int jj = i; jj < pa::NH; jj++) acc[pa::sym_index(i, jj)] += sd[i] * sd[jj];
                acc[pa::NSYM + i] += sd[i] * rd;
            }
            acc[pa::NSYM + pa::NH] += rd * rd;
            n_valid++;
        }
    }
#pragma unroll
    for (int k = 0; k < PA_ND; k++) {
        const double t = wave_sum(acc[k]);
        if (lane == 0) w_sum[wave * PA_ND + k] = t;
    }
    n_valid = wave_sum(n_valid);
    if (lane == 0) w_cnt[wave] = n_valid;
    __syncthreads();
    AlignSums* out = partial + (size_t)pair * PHOTO_SLICES + slice;
    if (tid < PA_ND) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < PA_WAVES; w++) t += w_sum[w * PA_ND + tid];
        reinterpret_cast<double*>(out)[tid] = t;
    } else if (tid == PA_ND) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < PA_WAVES; w++) t += w_cnt[w];
        out->n_valid = t;
        out->pad = 0;
    }
}

// grid: PHOTO_SLICES * n workgroups of pl_threads(L) (slice = block % PHOTO_SLICES).  pyr1 / pyr2: [n][PYR_BYTES].  x0 != nullptr: the level's first
// linearisation, at x0 [n][8]; otherwise at work[pair].x_trial, and a pair whose record OF THIS LEVEL carries a flag has stopped.
template <int L>
__global__ __launch_bounds__(pl_threads(L)) void photo_pyr_accum_kernel(const uint8_t* __restrict__ pyr1, const uint8_t* __restrict__ pyr2,
                                                                        const float* __restrict__ x0, const AlignWork* __restrict__ work,
                                                                        const AlignRec* __restrict__ rec, AlignSums* __restrict__ partial) {
    constexpr int W = pa::level_w(L), LPIX = pa::level_pix(L), SLICE_PIX = LPIX / PHOTO_SLICES, THREADS = pl_threads(L), WAVES = THREADS / 64;
    static_assert(L >= 1 && L < pa::MAX_LEVELS && pa::level_h(L) % PHOTO_SLICES == 0 && LPIX % 16 == 0 && pa::level_offset(L) % 16 == 0, "whole rows per slice");
    __shared__ __attribute__((aligned(16))) uint8_t tile[LPIX];
    __shared__ double w_sum[WAVES * PA_ND];
    __shared__ int w_cnt[WAVES];
    __shared__ float hs[9];
    const int pair = blockIdx.x / PHOTO_SLICES, slice = blockIdx.x - pair * PHOTO_SLICES;
    if (!x0 && rec[pair].flags != 0) return;                                  // (workgroup-uniform)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {
        const uint4* src = reinterpret_cast<const uint4*>(pyr2 + (size_t)pair * PYR_BYTES + pa::level_offset(L));
        for (int i = tid; i < LPIX / 16; i += THREADS) reinterpret_cast<uint4*>(tile)[i] = src[i];
    }
    if (tid == 0) {
        float h[9];
        pa_homography(x0 ? x0 + (size_t)pair * 8 : work[pair].x_trial, h);
#pragma unroll
        for (int k = 0; k < 9; k++) hs[k] = h[k];
    }
    __syncthreads();
    float h[9];
#pragma unroll
    for (int k = 0; k < 9; k++) h[k] = hs[k];

    const uint8_t* a_img = pyr1 + (size_t)pair * PYR_BYTES + pa::level_offset(L);
    double acc[PA_ND];
#pragma unroll
    for (int k = 0; k < PA_ND; k++) acc[k] = 0.0;
    int n_valid = 0;
    for (int i = tid; i < SLICE_PIX; i += THREADS) {
        const int pix = slice * SLICE_PIX + i;
        const int v = pix / W, u = pix - v * W;
        const float fu = pa::level_centre(L, u), fv = pa::level_centre(L, v);
        float ix0, iy0, Z, ix, iy;
        pa::level_coords(h, fu, fv, WarpDiv{}, ix0, iy0, Z);
        if (!pa::level_position(L, ix0, iy0, ix, iy)) continue;              // (false for NaN)
        const uint8_t* p = tile + (int)floorf(iy) * W + (int)floorf(ix);
        float r, s[pa::NH];
        pa::level_row(L, PixRead<uint8_t>::cvt(p[0]), PixRead<uint8_t>::cvt(p[1]), PixRead<uint8_t>::cvt(p[W]), PixRead<uint8_t>::cvt(p[W + 1]),
                      PixRead<uint8_t>::cvt(a_img[pix]), ix, iy, ix0, iy0, Z, fu, fv, r, s);
        double sd[pa::NH];
#pragma unroll
        for (int k = 0; k < pa::NH; k++) sd[k] = (double)s[k];
        const double rd = (double)r;
#pragma unroll
        for (int k = 0; k < pa::NH; k++) {
#pragma unroll
            for (int j = k; j < pa::NH; j++) acc[pa::sym_index(k, j)] += sd[k] * sd[j];
            acc[pa::NSYM + k] += sd[k] * rd;
        }
        acc[pa::NSYM + pa::NH] += rd * rd;
        n_valid++;
    }
#pragma unroll
    for (int k = 0; k < PA_ND; k++) {
        const double t = wave_sum(acc[k]);
        if (lane == 0) w_sum[wave * PA_ND + k] = t;
    }
    n_valid = wave_sum(n_valid);
    if (lane == 0) w_cnt[wave] = n_valid;
    __syncthreads();
    AlignSums* out = partial + (size_t)pair * PHOTO_SLICES + slice;
    if (tid < PA_ND) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) t += w_sum[w * PA_ND + tid];
        reinterpret_cast<double*>(out)[tid] = t;
    } else if (tid == PA_ND) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) t += w_cnt[w];
        out->n_valid = t;
        out->pad = 0;
    }
}
static_assert(PA_ND + 1 <= 64, "one wave writes a partial");

// grid: PHOTO_SLICES * n workgroups of pr_threads(L) (slice = block % PHOTO_SLICES).  img1 / img2: the level-L images of pair 0, `stride` bytes from a pair to
// the next (NPIX at level 0, PYR_BYTES above).  start != nullptr: the level's first linearisation, at start [n]; otherwise at work[pair]'s trial point, and a
// pair whose record OF THIS LEVEL carries a flag has stopped.
template <int L>
__global__ __launch_bounds__(pr_threads(L)) void photo_robust_accum_kernel(const uint8_t* __restrict__ img1, const uint8_t* __restrict__ img2, int stride,
                                                                           float kf, const RobustStart* __restrict__ start,
                                                                           const RobustWork* __restrict__ work, const RobustRec* __restrict__ rec,
                                                                           RobustSums* __restrict__ partial) {
    constexpr int W = pa::level_w(L), LPIX = pa::level_pix(L), SLICE_PIX = LPIX / PHOTO_SLICES, THREADS = pr_threads(L), WAVES = THREADS / 64;
    static_assert(L >= 0 && L < pa::MAX_LEVELS && pa::level_h(L) % PHOTO_SLICES == 0 && LPIX % 16 == 0 && pa::level_offset(L) % 16 == 0, "whole rows per slice");
    static_assert(L > 0 || (SLICE_PIX % (4 * THREADS) == 0 && W % 4 == 0), "whole quads per thread at level 0");
    extern __shared__ __attribute__((aligned(16))) uint8_t pr_lds[];
    const int pair = blockIdx.x / PHOTO_SLICES, slice = blockIdx.x - pair * PHOTO_SLICES;
    if (!start && rec[pair].px.flags != 0) return;                            // (workgroup-uniform)
    double* w_sum = reinterpret_cast<double*>(pr_lds + LPIX);
    int* w_cnt = reinterpret_cast<int*>(w_sum + WAVES * PR_ND);
    float* hs = reinterpret_cast<float*>(w_cnt + WAVES * 2);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {
        const uint4* src = reinterpret_cast<const uint4*>(img2 + (size_t)pair * stride);
        for (int i = tid; i < LPIX / 16; i += THREADS) reinterpret_cast<uint4*>(pr_lds)[i] = src[i];
    }
    if (tid == 0) {
        float h[9];
        pa_homography(start ? start[pair].x : work[pair].x_trial, h);
#pragma unroll
        for (int k = 0; k < 9; k++) hs[k] = h[k];
        hs[9] = pr::gain_f(start ? start[pair].gain : work[pair].gain_trial);
        hs[10] = pr::bias_f(start ? start[pair].bias : work[pair].bias_trial);
    }
    __syncthreads();
    float h[9];
#pragma unroll
    for (int k = 0; k < 9; k++) h[k] = hs[k];
    const float Gf = hs[9], bf = hs[10];

    const uint8_t* tile = pr_lds;
    const uint8_t* a_img = img1 + (size_t)pair * stride;
    double acc[PR_ND];
#pragma unroll
    for (int k = 0; k < PR_ND; k++) acc[k] = 0.0;
    int n_valid = 0, n_out = 0;
    if constexpr (L == 0) {
        const int pix0 = slice * SLICE_PIX + 4 * tid;
        for (int q = 0; q < SLICE_PIX / (4 * THREADS); q++) {
            const int pix = pix0 + q * (4 * THREADS);
            const int v = pix / W, u0 = pix - v * W;
            const uint32_t a4 = *reinterpret_cast<const uint32_t*>(a_img + pix);
            for (int j = 0; j < 4; j++)
                pr_pixel<L>(h, Gf, bf, kf, tile, u0 + j, v, PixRead<uint8_t>::cvt((uint8_t)(a4 >> (8 * j))), acc, n_valid, n_out);
        }
    } else {
        for (int i = tid; i < SLICE_PIX; i += THREADS) {
            const int pix = slice * SLICE_PIX + i;
            const int v = pix / W, u = pix - v * W;
            pr_pixel<L>(h, Gf, bf, kf, tile, u, v, PixRead<uint8_t>::cvt(a_img[pix]), acc, n_valid, n_out);
        }
    }
#pragma unroll
    for (int k = 0; k < PR_ND; k++) {
        const double t = wave_sum(acc[k]);
        if (lane == 0) w_sum[wave * PR_ND + k] = t;
    }
    n_valid = wave_sum(n_valid);
    n_out = wave_sum(n_out);
    if (lane == 0) { w_cnt[2 * wave] = n_valid; w_cnt[2 * wave + 1] = n_out; }
    __syncthreads();
    RobustSums* out = partial + (size_t)pair * PHOTO_SLICES + slice;
    for (int e = tid; e < PR_ND + 2; e += THREADS) {
        if (e < PR_ND) {
            double t = 0.0;
#pragma unroll
            for (int w = 0; w < WAVES; w++) t += w_sum[w * PR_ND + e];
            reinterpret_cast<double*>(out)[e] = t;
        } else {
            int t = 0;
#pragma unroll
            for (int w = 0; w < WAVES; w++) t += w_cnt[2 * w + (e - PR_ND)];
            (e == PR_ND ? out->n_valid : out->n_outliers) = t;
        }
    }
}

// grid: n workgroups of 64 lanes.  Linearisation `it` of the level (0: at x0) is in partial; the pair's record and work are read and written in place.
__global__ __launch_bounds__(64) void photo_align_solve_kernel(const AlignSums* __restrict__ partial, const float* __restrict__ x0, int it, AlignOpts opts,
                                                               AlignWork* work, AlignRec* rec) {
    __shared__ double sums[PA_ND], D[pa::NH * pa::NX], T[pa::NH * pa::NX], A[pa::NX * pa::NX], g[pa::NX], L[pa::NX * pa::NX];
    __shared__ int cnt[2], degenerate;
    const int pair = blockIdx.x, tid = threadIdx.x;
    if (it > 0 && rec[pair].flags != 0) return;                               // (workgroup-uniform: the pair has stopped)
    pa_solve_front<PA_ND>(partial + (size_t)pair * PHOTO_SLICES, it == 0 ? x0 + (size_t)pair * 8 : work[pair].x_trial, sums, cnt, &degenerate, D);
    pa_solve_T(sums, D, T);
    {
        const int i = tid / pa::NX, j = tid % pa::NX;
        if (i <= j) A[i * pa::NX + j] = A[j * pa::NX + i] = pa::form_A(D, T, i, j);
        if (tid < pa::NX) g[tid] = pa::form_g(D, sums + pa::NSYM, tid);
    }
    __syncthreads();
    if (tid == 0) pa::step(rec[pair], work[pair], it, opts, x0 + (size_t)pair * 8, degenerate != 0, cnt[0], sums[pa::NSYM + pa::NH], A, g, L);
}

// the same at start [n] with the ten parameters {x, gain, bias}
__global__ __launch_bounds__(64) void photo_robust_solve_kernel(const RobustSums* __restrict__ partial, const RobustStart* __restrict__ start, int it,
                                                                RobustOpts opts, RobustWork* work, RobustRec* rec) {
    __shared__ double sums[pr::ND], ss[pa::NSYM], D[pa::NH * pa::NX], T[pa::NH * pa::NX], A[pr::NP * pr::NP], g[pr::NP], Lc[pr::NP * pr::NP];
    __shared__ int cnt[2], degenerate;
    const int pair = blockIdx.x, tid = threadIdx.x;
    if (it > 0 && rec[pair].px.flags != 0) return;                            // (workgroup-uniform: the pair has stopped)
    const double G = it == 0 ? start[pair].gain : work[pair].gain_trial;
    pa_solve_front<pr::ND>(partial + (size_t)pair * PHOTO_SLICES, it == 0 ? start[pair].x : work[pair].x_trial, sums, cnt, &degenerate, D);
    if (tid < pa::NSYM) ss[tid] = pr::ss_entry(sums, tid);
    __syncthreads();
    pa_solve_T(ss, D, T);
    for (int e = tid; e < pr::NP * pr::NP; e += 64) {
        const int i = e / pr::NP, j = e % pr::NP;
        if (i <= j) A[i * pr::NP + j] = A[j * pr::NP + i] = pr::form_A10(D, sums, G, j < pa::NX ? pa::form_A(D, T, i, j) : 0.0, i, j);
    }
    if (tid < pr::NP) g[tid] = pr::form_g10(D, sums + pr::NSYM_T, G, tid);
    __syncthreads();
    if (tid == 0) pr::step(rec[pair], work[pair], it, opts, start[pair], degenerate != 0, cnt[0], cnt[1], sums[pr::NSYM_T + pr::NT], A, g, Lc);
}

// start [n][8] = rec[pair].offsets_px, as bits
__global__ __launch_bounds__(256) void photo_pyr_gather_kernel(const AlignRec* __restrict__ rec, uint32_t* __restrict__ start, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n * 8) start[i] = reinterpret_cast<const uint32_t*>(rec[i >> 3].offsets_px)[i & 7];
}

// start [n] as 12 words per pair: x [8] | gain | bias.  rec == nullptr: from the call's x0 [n][8] and gain0 / bias0; otherwise from the records of the level
// above, as bits
__global__ __launch_bounds__(256) void photo_robust_gather_kernel(const RobustRec* __restrict__ rec, const uint32_t* __restrict__ x0, double gain0, double bias0,
                                                                  uint32_t* __restrict__ start, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n * 12) return;
    const int pair = i / 12, k = i - pair * 12;
    uint32_t v;
    if (k < 8) {
        v = rec ? reinterpret_cast<const uint32_t*>(rec[pair].px.offsets_px)[k] : x0[pair * 8 + k];
    } else if (rec) {
        v = reinterpret_cast<const uint32_t*>(&rec[pair].gain)[k - 8];
    } else {
        const unsigned long long b = (unsigned long long)__double_as_longlong(k < 10 ? gain0 : bias0);
        v = (uint32_t)(b >> (32 * (k & 1)));
    }
    start[i] = v;
}
static_assert(sizeof(RobustStart) == 48 && offsetof(RobustStart, gain) == 32 && offsetof(RobustRec, bias) == offsetof(RobustRec, gain) + 8, "12 words per start");

namespace {

// What the level driver asks of a form of the alignment: its types, the base options, the level's start, one accumulate launch of level L and one solve launch.
struct PlainForm {
    using Opts = AlignOpts; using Start = float; using Sums = AlignSums; using Work = AlignWork; using Rec = AlignRec;      // (start: [n][8] offsets)
    template <class O> static O& base(O& o) { return o; }                      // (O: Opts or const Opts)
    // the call's x0 at the coarsest level (above == nullptr: no launch), the offsets the level above ended at below it
    static const float* gather(const Rec* above, const float* x0, const Opts&, float* start, int n, hipStream_t s) {
        if (!above) return x0;
        hipLaunchKernelGGL(photo_pyr_gather_kernel, dim3((unsigned)((n * 8 + 255) / 256)), dim3(256), 0, s, above, reinterpret_cast<uint32_t*>(start), n);
        return start;
    }
    template <int L>
    static void accumulate(const uint8_t* img1, const uint8_t* img2, const uint8_t* pyr1, const uint8_t* pyr2, int n, const float* start, const Opts&,
                           const Work* work, const Rec* rec, Sums* partial, hipStream_t s) {
        const dim3 grid((unsigned)(n * PHOTO_SLICES));
        if constexpr (L == 0) hipLaunchKernelGGL(photo_align_accum_kernel, grid, dim3(PA_THREADS), PA_LDS_BYTES, s, img1, img2, start, work, rec, partial);
        else hipLaunchKernelGGL(photo_pyr_accum_kernel<L>, grid, dim3(pl_threads(L)), 0, s, pyr1, pyr2, start, work, rec, partial);
    }
    static void solve(const Sums* partial, const float* start, int it, const Opts& o, int n, Work* work, Rec* rec, hipStream_t s) {
        hipLaunchKernelGGL(photo_align_solve_kernel, dim3((unsigned)n), dim3(64), 0, s, partial, start, it, o, work, rec);
    }
};
struct RobustForm {
    using Opts = RobustOpts; using Start = RobustStart; using Sums = RobustSums; using Work = RobustWork; using Rec = RobustRec;
    template <class O> static auto& base(O& o) { return o.base; }
    // one launch at every level
    static const Start* gather(const Rec* above, const float* x0, const Opts& o, Start* start, int n, hipStream_t s) {
        hipLaunchKernelGGL(photo_robust_gather_kernel, dim3((unsigned)((n * 12 + 255) / 256)), dim3(256), 0, s, above, reinterpret_cast<const uint32_t*>(x0), o.gain0,
                           o.bias0, reinterpret_cast<uint32_t*>(start), n);
        return start;
    }
    template <int L>
    static void accumulate(const uint8_t* img1, const uint8_t* img2, const uint8_t* pyr1, const uint8_t* pyr2, int n, const Start* start, const Opts& o,
                           const Work* work, const Rec* rec, Sums* partial, hipStream_t s) {
        hipLaunchKernelGGL(photo_robust_accum_kernel<L>, dim3((unsigned)(n * PHOTO_SLICES)), dim3(pr_threads(L)), pr_lds_bytes(L), s,
                           L == 0 ? img1 : pyr1 + pa::level_offset(L), L == 0 ? img2 : pyr2 + pa::level_offset(L), L == 0 ? NPIX : PYR_BYTES, pr::huber_f(o.huber_k),
                           start, work, rec, partial);
    }
    static void solve(const Sums* partial, const Start* start, int it, const Opts& o, int n, Work* work, Rec* rec, hipStream_t s) {
        hipLaunchKernelGGL(photo_robust_solve_kernel, dim3((unsigned)n), dim3(64), 0, s, partial, start, it, o, work, rec);
    }
};

// The robust form on the template pixels a mask admits: RobustForm's gather and solve, the accumulate launches of kernels_photo_masked.hip.
// The mask, its pyramid and its counts travel in the options, which the driver hands to every launch.
struct MaskedOpts { RobustOpts r; const uint8_t* mask0; const uint8_t* mpyr; const int32_t* n_mask; };
struct MaskedForm {
    using Opts = MaskedOpts; using Start = RobustStart; using Sums = RobustSums; using Work = RobustWork; using Rec = RobustRec;
    template <class O> static auto& base(O& o) { return o.r.base; }
    static const Start* gather(const Rec* above, const float* x0, const Opts& o, Start* start, int n, hipStream_t s) {
        return RobustForm::gather(above, x0, o.r, start, n, s);
    }
    template <int L>
    static void accumulate(const uint8_t* img1, const uint8_t* img2, const uint8_t* pyr1, const uint8_t* pyr2, int n, const Start* start, const Opts& o,
                           const Work* work, const Rec* rec, Sums* partial, hipStream_t s) {
        launch_photo_masked_accum(L, L == 0 ? img1 : pyr1 + pa::level_offset(L), L == 0 ? img2 : pyr2 + pa::level_offset(L),
                                  L == 0 ? o.mask0 : o.mpyr + pa::level_offset(L), o.n_mask, L == 0 ? NPIX : PYR_BYTES, n, pr::huber_f(o.r.huber_k), start, work,
                                  rec, partial, s);
    }
    static void solve(const Sums* partial, const Start* start, int it, const Opts& o, int n, Work* work, Rec* rec, hipStream_t s) {
        RobustForm::solve(partial, start, it, o.r, n, work, rec, s);
    }
};

// one level: max_iterations + 1 pairs of {accumulate, solve}
template <int L, class F>
hipError_t pa_run_level(const uint8_t* img1, const uint8_t* img2, const uint8_t* pyr1, const uint8_t* pyr2, int n, const typename F::Start* start,
                        const typename F::Opts& o, typename F::Sums* partial, typename F::Work* work, typename F::Rec* rec, hipStream_t s) {
    for (int it = 0; it <= F::base(o).max_iterations; it++) {
        F::template accumulate<L>(img1, img2, pyr1, pyr2, n, it == 0 ? start : nullptr, o, work, rec, partial, s);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        F::solve(partial, start, it, o, n, work, rec, s);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The launch sequence of one call: the pyramid (levels > 1), then per level from levels - 1 down to 0 the level's min_valid, its start and its iterations.
template <class F>
hipError_t pa_run_levels(const uint8_t* img1, const uint8_t* img2, int n, const float* x0, const typename F::Opts& opts, int levels, uint8_t* pyr1, uint8_t* pyr2,
                         typename F::Start* start, typename F::Sums* partial, typename F::Work* work, typename F::Rec* rec, hipStream_t s) {
    if (levels < 1 || levels > pa::MAX_LEVELS || n < 1 || n > (1 << 20) || !img1 || !img2 || !x0 || !partial || !work || !rec) return hipErrorInvalidValue;
    if ((((uintptr_t)img1) & 15) || (((uintptr_t)img2) & 15) || (levels > 1 && (!pyr1 || !pyr2 || !start))) return hipErrorInvalidValue;
    if (levels > 1) {
        const hipError_t e = launch_photo_pyramid(img1, img2, n, pyr1, pyr2, s);
        if (e != hipSuccess) return e;
    }
    for (int L = levels - 1; L >= 0; L--) {
        typename F::Opts o = opts;
        F::base(o).min_valid = pa::level_min_valid(F::base(o).min_valid, L);
        typename F::Rec* r = rec + (size_t)L * n;
        const typename F::Start* x = F::gather(L < levels - 1 ? r + n : nullptr, x0, opts, start, n, s);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        if (L == 0) e = pa_run_level<0, F>(img1, img2, pyr1, pyr2, n, x, o, partial, work, r, s);
        else if (L == 1) e = pa_run_level<1, F>(img1, img2, pyr1, pyr2, n, x, o, partial, work, r, s);
        else if (L == 2) e = pa_run_level<2, F>(img1, img2, pyr1, pyr2, n, x, o, partial, work, r, s);
        else e = pa_run_level<3, F>(img1, img2, pyr1, pyr2, n, x, o, partial, work, r, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t photo_align_init_device() {
    const hipError_t e = hipFuncSetAttribute((const void*)photo_align_accum_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PA_LDS_BYTES);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void*)photo_robust_accum_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, pr_lds_bytes(0));
}

hipError_t launch_photo_align_pyramid(const uint8_t* img1, const uint8_t* img2, int n, const float* x0, const AlignOpts& opts, int levels, uint8_t* pyr1,
                                      uint8_t* pyr2, float* start, AlignSums* partial, AlignWork* work, AlignRec* rec, hipStream_t s) {
    if (!pa::opts_valid(opts)) return hipErrorInvalidValue;
    return pa_run_levels<PlainForm>(img1, img2, n, x0, opts, levels, pyr1, pyr2, start, partial, work, rec, s);
}

hipError_t launch_photo_align_robust(const uint8_t* img1, const uint8_t* img2, int n, const float* x0, const RobustOpts& opts, int levels, uint8_t* pyr1,
                                     uint8_t* pyr2, RobustStart* start, RobustSums* partial, RobustWork* work, RobustRec* rec, hipStream_t s) {
    if (!start || !pr::opts_valid(opts)) return hipErrorInvalidValue;
    return pa_run_levels<RobustForm>(img1, img2, n, x0, opts, levels, pyr1, pyr2, start, partial, work, rec, s);
}

hipError_t launch_photo_align_masked(const uint8_t* img1, const uint8_t* mask1, const uint8_t* img2, int n, const float* x0, const RobustOpts& opts, int levels,
                                     uint8_t* pyr1, uint8_t* pyr2, uint8_t* mpyr, int32_t* n_mask, RobustStart* start, RobustSums* partial, RobustWork* work,
                                     RobustRec* rec, hipStream_t s) {
    if (!start || !pr::opts_valid(opts)) return hipErrorInvalidValue;
    const hipError_t e = launch_photo_mask_pyramid(mask1, n, mpyr, n_mask, s);
    if (e != hipSuccess) return e;
    return pa_run_levels<MaskedForm>(img1, img2, n, x0, MaskedOpts{opts, mask1, mpyr, n_mask}, levels, pyr1, pyr2, start, partial, work, rec, s);
}

}  // namespace hnet
