// kernels_photo_robust.hip — photometric alignment with a gain / bias model and Huber weights (photo_robust_dev.h, include/hnet.h
// hnet_op_photo_align_robust).  A third call beside kernels_photo_align.hip and kernels_photo_pyramid.hip, whose kernels this file does not touch;
// the pyramid is launch_photo_pyramid's.
//
// photo_robust_accum_kernel<L>, L = 0 .. 3: the contract of the existing accumulate kernels.  One workgroup of 256 / 256 / 128 / 64 threads per (row slice,
// pair), the pair's level-L img2 staged in LDS with 16-byte loads, lane 0 forms H, 78 double accumulators and two counts per thread (the 66 + 11 + 1 sums of
// include/hnet_photo_robust.h), lanes reduced by the fixed __shfl_down tree, the waves in wave order through LDS, one partial per slice, no floating-point
// atomics, and nothing waits on another workgroup.  Level 0 walks quads of 4 consecutive pixels as photo_align_accum_kernel does, levels 1 - 3 stride by the
// workgroup as photo_pyr_accum_kernel does: with the model off and huber_k = 0 every sum of the s block is made of the same terms in the same order as theirs,
// which is what makes the common part of a record equal theirs byte for byte.  The per-pixel quantity is the shared headers' (level_coords, level_position,
// level_row; sample, residual, weighted_row), the functions the host reference runs in a loop.
//
// photo_robust_solve_kernel (one workgroup of 64 lanes per pair) adds the 7 partials in slice order, forms D, T, A10 and g10 entry by entry over its lanes and
// lane 0 takes the step (hnet_robust::step).  photo_robust_gather_kernel writes a level's start {x, G, b}: from the call's start at the coarsest level, from
// the records of the level above (as bits: a NaN keeps its payload) below it.  Levels and iterations are separate launches.
#include "photo_robust_dev.h"
#include "warp_dev.h"

namespace hnet {

namespace pa = hnet_align;
namespace pr = hnet_robust;

namespace {
constexpr int PR_ND = pr::ND;                                                    // 78
constexpr int pr_threads(int L) { return L <= 1 ? 256 : (L == 2 ? 128 : 64); }
// dynamic LDS of the accumulate kernel: img2 of the level | per-wave sums [waves][78] f64 | per-wave counts [waves][2] i32 | H [9], Gf, bf, kf f32
constexpr int pr_lds_bytes(int L) { return pa::level_pix(L) + (pr_threads(L) / 64) * (PR_ND * 8 + 8) + 12 * 4; }
static_assert(2 * pr_lds_bytes(0) <= 160 * 1024, "two level-0 workgroups share a CU's LDS");
static_assert(offsetof(RobustSums, tr) == pr::NSYM_T * 8 && offsetof(RobustSums, rho) == (pr::NSYM_T + pr::NT) * 8 && offsetof(RobustSums, n_valid) == PR_ND * 8 &&
              offsetof(RobustSums, n_outliers) == PR_ND * 8 + 4, "RobustSums is 78 doubles, then the two counts");

// warp_coords' quotients (csrc/warp_dev.h): the reciprocal form where Z is far from the ends of the exponent range, the compiler's division elsewhere
struct WarpDiv {
    __device__ __forceinline__ void operator()(float X, float Y, float Z, float& qx, float& qy) const {
        if (warp_z_safe(Z)) {
            const float r1 = warp_rcp_refined(Z);
            qx = warp_div_with(X, Z, r1);
            qy = warp_div_with(Y, Z, r1);
        } else {
            qx = X / Z;
            qy = Y / Z;
        }
    }
};

// one pixel (u, v) of level L into the thread's accumulators; i1: the level-L img1 pixel as u8 / 255
template <int L>
__device__ __forceinline__ void pr_pixel(const float* h, float Gf, float bf, float kf, const uint8_t* tile, int u, int v, float i1, double (&acc)[PR_ND],
                                         int& n_valid, int& n_out) {
    constexpr int W = pa::level_w(L);
    const float fu = pa::level_centre(L, u), fv = pa::level_centre(L, v);
    float ix0, iy0, Z, ix, iy;
    pa::level_coords(h, fu, fv, WarpDiv{}, ix0, iy0, Z);
    if (!pa::level_position(L, ix0, iy0, ix, iy)) return;                    // (false for NaN)
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
}  // namespace

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
        const double t = pa_wave_sum(acc[k]);
        if (lane == 0) w_sum[wave * PR_ND + k] = t;
    }
    n_valid = pa_wave_sum(n_valid);
    n_out = pa_wave_sum(n_out);
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

// grid: n workgroups of 64 lanes.  Linearisation `it` of the level (0: at start) is in partial; the pair's record and work are read and written in place.
__global__ __launch_bounds__(64) void photo_robust_solve_kernel(const RobustSums* __restrict__ partial, const RobustStart* __restrict__ start, int it,
                                                                RobustOpts opts, RobustWork* work, RobustRec* rec) {
    __shared__ double sums[PR_ND], ss[pa::NSYM], D[pa::NH * pa::NX], T[pa::NH * pa::NX], A[pr::NP * pr::NP], g[pr::NP], Lc[pr::NP * pr::NP];
    __shared__ int cnt[2], degenerate;
    const int pair = blockIdx.x, tid = threadIdx.x;
    if (it > 0 && rec[pair].px.flags != 0) return;                            // (workgroup-uniform: the pair has stopped)
    const float* x = it == 0 ? start[pair].x : work[pair].x_trial;
    const double G = it == 0 ? start[pair].gain : work[pair].gain_trial;
    const RobustSums* part = partial + (size_t)pair * PHOTO_SLICES;
    for (int e = tid; e < PR_ND + 2; e += 64) {
        if (e < PR_ND) {
            double t = 0.0;
#pragma unroll
            for (int s = 0; s < PHOTO_SLICES; s++) t += reinterpret_cast<const double*>(part + s)[e];
            sums[e] = t;
        } else {
            int t = 0;
#pragma unroll
            for (int s = 0; s < PHOTO_SLICES; s++) t += e == PR_ND ? part[s].n_valid : part[s].n_outliers;
            cnt[e - PR_ND] = t;
        }
    }
    if (tid == 63) {
        float h[9];
        degenerate = pa_homography(x, h) ? 0 : 1;
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
    if (tid < pa::NSYM) ss[tid] = pr::ss_entry(sums, tid);
    __syncthreads();
    for (int e = tid; e < pa::NH * pa::NX; e += 64) T[e] = pa::form_T(ss, D, e / pa::NX, e % pa::NX);
    __syncthreads();
    for (int e = tid; e < pr::NP * pr::NP; e += 64) {
        const int i = e / pr::NP, j = e % pr::NP;
        if (i <= j) A[i * pr::NP + j] = A[j * pr::NP + i] = pr::form_A10(D, sums, G, j < pa::NX ? pa::form_A(D, T, i, j) : 0.0, i, j);
    }
    if (tid < pr::NP) g[tid] = pr::form_g10(D, sums + pr::NSYM_T, G, tid);
    __syncthreads();
    if (tid == 0) pr::step(rec[pair], work[pair], it, opts, start[pair], degenerate != 0, cnt[0], cnt[1], sums[pr::NSYM_T + pr::NT], A, g, Lc);
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

hipError_t photo_robust_init_device() {
    return hipFuncSetAttribute((const void*)photo_robust_accum_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, pr_lds_bytes(0));
}

namespace {
template <int L>
hipError_t launch_level(const uint8_t* img1, const uint8_t* img2, int stride, int n, const RobustStart* start, const RobustOpts& o, RobustSums* partial,
                        RobustWork* work, RobustRec* rec, hipStream_t s) {
    const float kf = pr::huber_f(o.huber_k);
    for (int it = 0; it <= o.base.max_iterations; it++) {
        hipLaunchKernelGGL(photo_robust_accum_kernel<L>, dim3((unsigned)(n * PHOTO_SLICES)), dim3(pr_threads(L)), pr_lds_bytes(L), s, img1, img2, stride, kf,
                           it == 0 ? start : nullptr, (const RobustWork*)work, (const RobustRec*)rec, partial);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(photo_robust_solve_kernel, dim3((unsigned)n), dim3(64), 0, s, (const RobustSums*)partial, start, it, o, work, rec);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
}  // namespace

hipError_t launch_photo_align_robust(const uint8_t* img1, const uint8_t* img2, int n, const float* x0, const RobustOpts& opts, int levels, uint8_t* pyr1,
                                     uint8_t* pyr2, RobustStart* start, RobustSums* partial, RobustWork* work, RobustRec* rec, hipStream_t s) {
    if (levels < 1 || levels > pa::MAX_LEVELS || n < 1 || n > (1 << 20) || !img1 || !img2 || !x0 || !start || !partial || !work || !rec || !pr::opts_valid(opts))
        return hipErrorInvalidValue;
    if ((((uintptr_t)img1) & 15) || (((uintptr_t)img2) & 15) || (levels > 1 && (!pyr1 || !pyr2))) return hipErrorInvalidValue;
    if (levels > 1) {
        const hipError_t e = launch_photo_pyramid(img1, img2, n, pyr1, pyr2, s);
        if (e != hipSuccess) return e;
    }
    for (int L = levels - 1; L >= 0; L--) {
        RobustOpts o = opts;
        o.base.min_valid = pa::level_min_valid(opts.base.min_valid, L);
        RobustRec* r = rec + (size_t)L * n;
        hipLaunchKernelGGL(photo_robust_gather_kernel, dim3((unsigned)((n * 12 + 255) / 256)), dim3(256), 0, s, L < levels - 1 ? (const RobustRec*)(r + n) : nullptr,
                           reinterpret_cast<const uint32_t*>(x0), opts.gain0, opts.bias0, reinterpret_cast<uint32_t*>(start), n);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        const uint8_t* a = L == 0 ? img1 : pyr1 + pa::level_offset(L);
        const uint8_t* b = L == 0 ? img2 : pyr2 + pa::level_offset(L);
        const int stride = L == 0 ? NPIX : PYR_BYTES;
        if (L == 0) e = launch_level<0>(a, b, stride, n, start, o, partial, work, r, s);
        else if (L == 1) e = launch_level<1>(a, b, stride, n, start, o, partial, work, r, s);
        else if (L == 2) e = launch_level<2>(a, b, stride, n, start, o, partial, work, r, s);
        else e = launch_level<3>(a, b, stride, n, start, o, partial, work, r, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace hnet
