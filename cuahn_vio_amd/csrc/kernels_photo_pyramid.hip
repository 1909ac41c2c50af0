// kernels_photo_pyramid.hip — the image pyramid and the coarse levels of photometric alignment (photo_pyramid_dev.h, include/hnet.h
// hnet_op_photo_align_pyramid).  Level 0 stays on kernels_photo_align.hip, whose kernels this file does not touch.
//
// photo_pyramid_kernel: ONE launch per call makes levels 1, 2, 3 of every frame.  A workgroup of 320 threads owns a band of 32 rows of one frame: each thread
// reads 16 pixels of two adjacent rows with two 16-byte loads (level 0 is read once), writes its 8 level-1 pixels to global memory and to LDS; level 2 is
// made from the ROUNDED level 1 in LDS, level 3 from level 2 in LDS (hnet_align::down4: exact integers, bit-identical to the host reference).
//
// photo_pyr_accum_kernel<L>: photo_align_accum_kernel's contract on the level-L images.  One workgroup per (row slice, pair), the pair's level-L img2 staged
// in LDS with 16-byte loads (17 920, 4 480 or 1 120 bytes), pixels of the slice taken in ascending order with a stride of the workgroup, 55 double
// accumulators and the count per thread, lanes reduced by a fixed __shfl_down tree, the waves in wave order through LDS, one partial per slice and no
// floating-point atomics: a record depends on its pair, start and options alone.  112, 56 and 28 rows divide by PHOTO_SLICES = 7, so
// photo_align_solve_kernel adds the 7 partials of every level unchanged.  The per-pixel quantity is include/hnet_photo_pyramid.h's (level_coords,
// level_position, level_row), the functions the host reference runs in a loop; the division is warp_coords' reciprocal form, bit-identical to IEEE x / z.
// As at level 0 a product of two floats is exact in a double: the device and the host reference differ in the ORDER of the additions only.
//
// The start offsets of a level are the offsets the level above ended at, whatever its flags: photo_pyr_gather_kernel copies them (as bits) from the records
// [n] of 656 bytes into the contiguous [n][8] the accumulate and solve kernels read.  Levels and iterations are separate launches; nothing waits on another
// workgroup, and a stopped pair's workgroups return at once (a workgroup-uniform branch).
#include "photo_pyramid_dev.h"
#include "warp_dev.h"

namespace hnet {

namespace pa = hnet_align;

namespace {
constexpr int PYR_BANDS = 7, PYR_BAND_ROWS = IMG_H / PYR_BANDS;               // 32 rows of level 0 -> 16, 8, 4 rows of levels 1, 2, 3
constexpr int PYR_THREADS = (PYR_BAND_ROWS / 2) * (IMG_W / 16);                // 320: one thread per 16 pixels of a pair of rows
static_assert(PYR_BAND_ROWS % 8 == 0 && IMG_W % 16 == 0 && PYR_THREADS == 320 && PYR_THREADS >= (PYR_BAND_ROWS / 8) * (IMG_W / 8), "a band holds whole 8 x 8 blocks");

// two pixels of the next level from four bytes of the upper and four of the lower row
__device__ __forceinline__ uint32_t pyr_down2(uint32_t t, uint32_t b) {
    const uint32_t lo = pa::down4(t & 0xFFu, (t >> 8) & 0xFFu, b & 0xFFu, (b >> 8) & 0xFFu);
    const uint32_t hi = pa::down4((t >> 16) & 0xFFu, t >> 24, (b >> 16) & 0xFFu, b >> 24);
    return lo | (hi << 8);
}
__device__ __forceinline__ uint32_t pyr_down4(uint32_t t0, uint32_t t1, uint32_t b0, uint32_t b1) { return pyr_down2(t0, b0) | (pyr_down2(t1, b1) << 16); }
}  // namespace

// grid: (PYR_BANDS, frames).  Frame f < n is img_a's, frame f >= n is img_b's frame f - n (img_b may be null when the grid has n frames only).
__global__ __launch_bounds__(PYR_THREADS) void photo_pyramid_kernel(const uint8_t* __restrict__ img_a, const uint8_t* __restrict__ img_b, int n,
                                                                    uint8_t* __restrict__ pyr_a, uint8_t* __restrict__ pyr_b) {
    constexpr int W1 = pa::level_w(1), W2 = pa::level_w(2), W3 = pa::level_w(3);
    __shared__ __attribute__((aligned(16))) uint8_t l1[(PYR_BAND_ROWS / 2) * W1];      // 16 x 160
    __shared__ __attribute__((aligned(16))) uint8_t l2[(PYR_BAND_ROWS / 4) * W2];      // 8 x 80
    const int band = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    const uint8_t* src = f < n ? img_a + (size_t)f * NPIX : img_b + (size_t)(f - n) * NPIX;
    uint8_t* dst = f < n ? pyr_a + (size_t)f * PYR_BYTES : pyr_b + (size_t)(f - n) * PYR_BYTES;
    {
        const int r = tid / (IMG_W / 16), cx = tid - r * (IMG_W / 16);          // row pair 0 .. 15, 16-pixel column 0 .. 19
        const uint8_t* p = src + (size_t)(band * PYR_BAND_ROWS + 2 * r) * IMG_W + cx * 16;
        const uint4 t = *reinterpret_cast<const uint4*>(p), b = *reinterpret_cast<const uint4*>(p + IMG_W);
        const uint2 o = make_uint2(pyr_down4(t.x, t.y, b.x, b.y), pyr_down4(t.z, t.w, b.z, b.w));
        *reinterpret_cast<uint2*>(l1 + r * W1 + cx * 8) = o;
        *reinterpret_cast<uint2*>(dst + pa::level_offset(1) + (band * (PYR_BAND_ROWS / 2) + r) * W1 + cx * 8) = o;
    }
    __syncthreads();
    if (tid < (PYR_BAND_ROWS / 4) * (W1 / 8)) {                                  // 8 rows x 20 groups of 4 level-2 pixels
        const int r = tid / (W1 / 8), cx = tid - r * (W1 / 8);
        const uint2 t = *reinterpret_cast<const uint2*>(l1 + (2 * r) * W1 + cx * 8), b = *reinterpret_cast<const uint2*>(l1 + (2 * r + 1) * W1 + cx * 8);
        const uint32_t o = pyr_down4(t.x, t.y, b.x, b.y);
        *reinterpret_cast<uint32_t*>(l2 + r * W2 + cx * 4) = o;
        *reinterpret_cast<uint32_t*>(dst + pa::level_offset(2) + (band * (PYR_BAND_ROWS / 4) + r) * W2 + cx * 4) = o;
    }
    __syncthreads();
    if (tid < (PYR_BAND_ROWS / 8) * W3) {                                        // 4 rows x 40 level-3 pixels
        const int r = tid / W3, c = tid - r * W3;
        const uint8_t* q = l2 + (2 * r) * W2 + 2 * c;
        dst[pa::level_offset(3) + (band * (PYR_BAND_ROWS / 8) + r) * W3 + c] = pa::down4(q[0], q[1], q[W2], q[W2 + 1]);
    }
}

namespace {
constexpr int pl_threads(int L) { return L == 1 ? 256 : (L == 2 ? 128 : 64); }  // 10, 5 and 2.5 pixels per thread and slice

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
}  // namespace

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

// start [n][8] = rec[pair].offsets_px, as bits (a NaN keeps its payload)
__global__ __launch_bounds__(256) void photo_pyr_gather_kernel(const AlignRec* __restrict__ rec, uint32_t* __restrict__ start, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n * 8) start[i] = reinterpret_cast<const uint32_t*>(rec[i >> 3].offsets_px)[i & 7];
}

hipError_t launch_photo_pyramid(const uint8_t* img_a, const uint8_t* img_b, int n, uint8_t* pyr_a, uint8_t* pyr_b, hipStream_t s) {
    if (n < 1 || n >= (1 << 15) || !img_a || !pyr_a || (img_b != nullptr) != (pyr_b != nullptr)) return hipErrorInvalidValue;      // (2 n frames in grid.y)
    if ((((uintptr_t)img_a) & 15) || (((uintptr_t)img_b) & 15) || (((uintptr_t)pyr_a) & 15) || (((uintptr_t)pyr_b) & 15)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(photo_pyramid_kernel, dim3(PYR_BANDS, (unsigned)(img_b ? 2 * n : n)), dim3(PYR_THREADS), 0, s, img_a, img_b, n, pyr_a, pyr_b);
    return hipGetLastError();
}

namespace {
template <int L>
hipError_t launch_level(const uint8_t* pyr1, const uint8_t* pyr2, int n, const float* x0, const AlignOpts& o, AlignSums* partial, AlignWork* work, AlignRec* rec,
                        hipStream_t s) {
    for (int it = 0; it <= o.max_iterations; it++) {
        hipLaunchKernelGGL(photo_pyr_accum_kernel<L>, dim3((unsigned)(n * PHOTO_SLICES)), dim3(pl_threads(L)), 0, s, pyr1, pyr2, it == 0 ? x0 : nullptr,
                           (const AlignWork*)work, (const AlignRec*)rec, partial);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        e = launch_photo_align_solve(partial, x0, it, o, n, work, rec, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
}  // namespace

hipError_t launch_photo_align_pyramid(const uint8_t* img1, const uint8_t* img2, int n, const float* x0, const AlignOpts& opts, int levels, uint8_t* pyr1,
                                      uint8_t* pyr2, float* start, AlignSums* partial, AlignWork* work, AlignRec* rec, hipStream_t s) {
    if (levels < 1 || levels > pa::MAX_LEVELS || n < 1 || n > (1 << 20) || !x0 || (levels > 1 && !start) || !partial || !work || !rec || !pa::opts_valid(opts))
        return hipErrorInvalidValue;
    if (levels > 1) {
        const hipError_t e = launch_photo_pyramid(img1, img2, n, pyr1, pyr2, s);
        if (e != hipSuccess) return e;
    }
    for (int L = levels - 1; L >= 0; L--) {
        AlignOpts o = opts;
        o.min_valid = pa::level_min_valid(opts.min_valid, L);
        AlignRec* r = rec + (size_t)L * n;
        const float* x = x0;
        if (L < levels - 1) {
            hipLaunchKernelGGL(photo_pyr_gather_kernel, dim3((unsigned)((n * 8 + 255) / 256)), dim3(256), 0, s, (const AlignRec*)(r + n),
                               reinterpret_cast<uint32_t*>(start), n);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
            x = start;
        }
        hipError_t e;
        if (L == 0) e = launch_photo_align(img1, img2, n, x, o, partial, work, r, s);
        else if (L == 1) e = launch_level<1>(pyr1, pyr2, n, x, o, partial, work, r, s);
        else if (L == 2) e = launch_level<2>(pyr1, pyr2, n, x, o, partial, work, r, s);
        else e = launch_level<3>(pyr1, pyr2, n, x, o, partial, work, r, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace hnet
