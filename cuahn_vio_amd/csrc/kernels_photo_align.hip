// kernels_photo_align.hip — photometric alignment on the four corner offsets (photo_align_dev.h, include/hnet.h hnet_photo_align).
//
// Forward-additive Lucas-Kanade / Levenberg-Marquardt on the squared form of the residual kernels_photo.hip sums.  One linearisation at offsets x is, over
// the VALID pixels (0 <= ix < 319, 0 <= iy < 223: all four bilinear taps are pixels of img2), the 45 + 9 + 1 sums and the count of
// include/hnet_photo_align.h: sum s s^T, sum s r, sum r^2 for r = (w - img1 / 255) * 255 and s = dr / dvec(H).  w is formed from the same four taps, the
// same u8 -> float conversion and the same FMA chain as warp_taps_global, at the position warp_coords gives: |r| has the bits of the error map.
//
// photo_align_accum_kernel has the form of photo_residual_kernel: one workgroup of 256 threads per (row slice, pair), the pair's img2 staged once in LDS with
// 16-byte loads, quads of 4 consecutive pixels per thread in ascending order, 56 accumulators per thread (55 doubles and the count), lanes reduced by a fixed
// __shfl_down tree, the 4 waves in wave order through LDS, one partial per slice.  No floating-point atomics: a pair's sums depend on the pair alone.
// photo_align_solve_kernel (one workgroup of 64 lanes per pair) adds the 7 partials in slice order, forms D, A = D^T (sum s s^T) D and g entry by entry
// over its lanes (hnet_align::form_T / form_A / form_g: the host reference runs the same functions in a loop) and lane 0 takes the step
// (hnet_align::step).  Iterations are separate launches: nothing here waits on another workgroup.
//
// Departures from the form the residual kernel set, and why:
//  - the trial H is not written by the solve kernel as nine floats: it writes the trial OFFSETS (32 bytes) and lane 0 of every accumulate workgroup forms
//    H = (float) dlt_solve(p4 + x) where photo_slice_body forms it.  One code path for the start offsets and the trials, and H is by construction the
//    matrix a residual record of the same offsets used.
//  - a product (double) s_i * (double) s_j of two floats is exact in a double, so contraction cannot change a sum: the device and the host reference
//    differ in the ORDER of the additions only.
#include "photo_align_dev.h"
#include "warp_dev.h"

namespace hnet {

namespace pa = hnet_align;

namespace {
constexpr int PA_THREADS = 256, PA_WAVES = PA_THREADS / 64;
constexpr int PA_QUADS = PHOTO_SLICE_PIX / (4 * PA_THREADS);                  // 10 quads per thread
static_assert(offsetof(AlignSums, sr) == pa::NSYM * 8 && offsetof(AlignSums, rr) == (pa::NSYM + pa::NH) * 8 && offsetof(AlignSums, n_valid) == PA_ND * 8,
              "AlignSums is 55 doubles, then the count");
// dynamic LDS of the accumulate kernel: img2 | per-wave sums [4][55] f64 | per-wave counts [4] i32 | H [9] f32 | flag
constexpr int PA_LDS_BYTES = NPIX + PA_WAVES * PA_ND * 8 + PA_WAVES * 4 + 9 * 4 + 4;      // 73 496: two workgroups per CU
static_assert(NPIX % 16 == 0 && 2 * PA_LDS_BYTES <= 160 * 1024, "aligned sections; two workgroups share a CU's LDS");

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
        const double t = pa_wave_sum(acc[k]);
        if (lane == 0) w_sum[wave * PA_ND + k] = t;
    }
    n_valid = pa_wave_sum(n_valid);
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

// grid: n workgroups of 64 lanes.  Linearisation `it` of the call (0: at x0) is in partial; the pair's record and work are read and written in place.
__global__ __launch_bounds__(64) void photo_align_solve_kernel(const AlignSums* __restrict__ partial, const float* __restrict__ x0, int it, AlignOpts opts,
                                                               AlignWork* work, AlignRec* rec) {
    __shared__ double sums[PA_ND], D[pa::NH * pa::NX], T[pa::NH * pa::NX], A[pa::NX * pa::NX], g[pa::NX], L[pa::NX * pa::NX];
    __shared__ int n_valid, degenerate;
    const int pair = blockIdx.x, tid = threadIdx.x;
    if (it > 0 && rec[pair].flags != 0) return;                               // (workgroup-uniform: the pair has stopped)
    const float* x = it == 0 ? x0 + (size_t)pair * 8 : work[pair].x_trial;
    const AlignSums* part = partial + (size_t)pair * PHOTO_SLICES;
    if (tid < PA_ND) {
        double t = 0.0;
#pragma unroll
        for (int s = 0; s < PHOTO_SLICES; s++) t += reinterpret_cast<const double*>(part + s)[tid];
        sums[tid] = t;
    } else if (tid == PA_ND) {
        int t = 0;
#pragma unroll
        for (int s = 0; s < PHOTO_SLICES; s++) t += part[s].n_valid;
        n_valid = t;
    } else if (tid == PA_ND + 1) {
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
    for (int e = tid; e < pa::NH * pa::NX; e += 64) T[e] = pa::form_T(sums, D, e / pa::NX, e % pa::NX);
    __syncthreads();
    {
        const int i = tid / pa::NX, j = tid % pa::NX;
        if (i <= j) A[i * pa::NX + j] = A[j * pa::NX + i] = pa::form_A(D, T, i, j);
        if (tid < pa::NX) g[tid] = pa::form_g(D, sums + pa::NSYM, tid);
    }
    __syncthreads();
    if (tid == 0) pa::step(rec[pair], work[pair], it, opts, x0 + (size_t)pair * 8, degenerate != 0, n_valid, sums[pa::NSYM + pa::NH], A, g, L);
}

static_assert(PHOTO_SLICES == 7 && PA_ND + 2 <= 64, "the solve kernel's lanes cover the sums, the count and the homography test");

hipError_t photo_align_init_device() {
    return hipFuncSetAttribute((const void*)photo_align_accum_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PA_LDS_BYTES);
}

hipError_t launch_photo_align_solve(const AlignSums* partial, const float* x0, int it, const AlignOpts& opts, int n, AlignWork* work, AlignRec* rec, hipStream_t s) {
    hipLaunchKernelGGL(photo_align_solve_kernel, dim3((unsigned)n), dim3(64), 0, s, partial, x0, it, opts, work, rec);
    return hipGetLastError();
}

hipError_t launch_photo_align(const uint8_t* img1, const uint8_t* img2, int n, const float* x0, const AlignOpts& opts, AlignSums* partial, AlignWork* work,
                              AlignRec* rec, hipStream_t s) {
    if (n < 1 || n > (1 << 20) || !img1 || !img2 || !x0 || !partial || !work || !rec || !pa::opts_valid(opts)) return hipErrorInvalidValue;
    if ((((uintptr_t)img1) & 3) || (((uintptr_t)img2) & 15)) return hipErrorInvalidValue;
    for (int it = 0; it <= opts.max_iterations; it++) {
        hipLaunchKernelGGL(photo_align_accum_kernel, dim3((unsigned)(n * PHOTO_SLICES)), dim3(PA_THREADS), PA_LDS_BYTES, s, img1, img2, it == 0 ? x0 : nullptr,
                           (const AlignWork*)work, (const AlignRec*)rec, partial);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        e = launch_photo_align_solve(partial, x0, it, opts, n, work, rec, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace hnet
