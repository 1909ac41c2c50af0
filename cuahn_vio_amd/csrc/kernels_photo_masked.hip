// kernels_photo_masked.hip — the robust photometric alignment on the template pixels a mask admits (photo_masked_dev.h, include/hnet.h
// hnet_op_photo_align_masked).  The rule is include/hnet_photo_masked.h's; the gather and solve kernels and the level driver are
// kernels_photo_align.hip's, which launches the kernels below through its third form.
//
// photo_mask_pyramid_kernel: ONE launch per call makes levels 1, 2, 3 of every mask (bytes 0 / 1: the AND of the 4^L level-0 bytes under a pixel) and the
// counts n_mask [4][7].  photo_pyramid_kernel's shape: a workgroup of 320 threads owns a band of 32 rows of one mask - the row slice of the accumulate
// launches at every level, so a workgroup writes its own four counts and waits on no other.  The counts go through the lanes' shuffle tree and the waves'
// words in LDS, in integers; no atomics.
//
// photo_masked_accum_kernel<0..3>: photo_robust_accum_kernel<L> (same threads, LDS layout, pr_pixel, shuffle tree and wave order: photo_robust_kernel_dev.h)
// with the mask in front of every pixel.  At level 0 a thread loads the four mask bytes of its quad as one word beside the four img1 bytes and skips the quad
// when the word is 0, a pixel when its byte is 0 (pr_pixel's `take`, one condition with its validity test); above level 0 it reads one byte per pixel.  A workgroup whose slice has no mask pixel at its level writes a
// zero partial, every byte, and returns BEFORE it stages img2 (a workgroup-uniform branch on n_mask).  A skipped pixel adds nothing, and the additions that
// remain keep the robust kernel's order: a mask without a zero byte gives the robust call's records bit for bit.  No floating-point atomics, no scratch.
#include "photo_masked_dev.h"
#include "photo_robust_kernel_dev.h"

namespace hnet {

namespace pa = hnet_align;
namespace pr = hnet_robust;
namespace pm = hnet_masked;

namespace {
constexpr int MK_BAND_ROWS = IMG_H / PHOTO_SLICES;                           // 32 rows of level 0 -> 16, 8, 4 rows of levels 1, 2, 3
constexpr int MK_THREADS = (MK_BAND_ROWS / 2) * (IMG_W / 16), MK_WAVES = MK_THREADS / 64;      // 320: one thread per 16 bytes of a pair of rows
static_assert(MK_BAND_ROWS % 8 == 0 && IMG_W % 16 == 0 && MK_THREADS == 320 && MK_THREADS % 64 == 0 && MK_THREADS >= (MK_BAND_ROWS / 8) * (IMG_W / 8),
              "a band holds whole 8 x 8 blocks; whole waves");
static_assert(pm::slice_rows(0) == MK_BAND_ROWS && pa::MAX_LEVELS == 4, "a band is a row slice at every level");

// the non-zero bytes of a word
__device__ __forceinline__ int mk_count(uint32_t w) {
    return ((w & 0xFFu) != 0u ? 1 : 0) + ((w & 0xFF00u) != 0u ? 1 : 0) + ((w & 0xFF0000u) != 0u ? 1 : 0) + ((w & 0xFF000000u) != 0u ? 1 : 0);
}
// two bytes of the next level from four bytes of the upper and four of the lower row
__device__ __forceinline__ uint32_t mk_and2(uint32_t t, uint32_t b) {
    const uint32_t lo = pm::and4(t & 0xFFu, (t >> 8) & 0xFFu, b & 0xFFu, (b >> 8) & 0xFFu);
    const uint32_t hi = pm::and4((t >> 16) & 0xFFu, t >> 24, (b >> 16) & 0xFFu, b >> 24);
    return lo | (hi << 8);
}
__device__ __forceinline__ uint32_t mk_and4(uint32_t t0, uint32_t t1, uint32_t b0, uint32_t b1) { return mk_and2(t0, b0) | (mk_and2(t1, b1) << 16); }
}  // namespace

// grid: (PHOTO_SLICES, n).  mask [n][NPIX] -> mpyr [n][PYR_BYTES], n_mask [n][N_MASK]
__global__ __launch_bounds__(MK_THREADS) void photo_mask_pyramid_kernel(const uint8_t* __restrict__ mask, uint8_t* __restrict__ mpyr, int32_t* __restrict__ n_mask) {
    constexpr int W1 = pa::level_w(1), W2 = pa::level_w(2), W3 = pa::level_w(3);
    __shared__ __attribute__((aligned(16))) uint8_t l1[(MK_BAND_ROWS / 2) * W1];      // 16 x 160
    __shared__ __attribute__((aligned(16))) uint8_t l2[(MK_BAND_ROWS / 4) * W2];      // 8 x 80
    __shared__ int w_cnt[MK_WAVES * pa::MAX_LEVELS];
    const int band = blockIdx.x, f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* src = mask + (size_t)f * NPIX;
    uint8_t* dst = mpyr + (size_t)f * PYR_BYTES;
    int cnt[pa::MAX_LEVELS] = {0, 0, 0, 0};
    {
        const int r = tid / (IMG_W / 16), cx = tid - r * (IMG_W / 16);          // row pair 0 .. 15, 16-byte column 0 .. 19
        const uint8_t* p = src + (size_t)(band * MK_BAND_ROWS + 2 * r) * IMG_W + cx * 16;
        const uint4 t = *reinterpret_cast<const uint4*>(p), b = *reinterpret_cast<const uint4*>(p + IMG_W);
        cnt[0] = mk_count(t.x) + mk_count(t.y) + mk_count(t.z) + mk_count(t.w) + mk_count(b.x) + mk_count(b.y) + mk_count(b.z) + mk_count(b.w);
        const uint2 o = make_uint2(mk_and4(t.x, t.y, b.x, b.y), mk_and4(t.z, t.w, b.z, b.w));
        cnt[1] = mk_count(o.x) + mk_count(o.y);
        *reinterpret_cast<uint2*>(l1 + r * W1 + cx * 8) = o;
        *reinterpret_cast<uint2*>(dst + pa::level_offset(1) + (band * (MK_BAND_ROWS / 2) + r) * W1 + cx * 8) = o;
    }
    __syncthreads();
    if (tid < (MK_BAND_ROWS / 4) * (W1 / 8)) {                                   // 8 rows x 20 groups of 4 level-2 bytes
        const int r = tid / (W1 / 8), cx = tid - r * (W1 / 8);
        const uint2 t = *reinterpret_cast<const uint2*>(l1 + (2 * r) * W1 + cx * 8), b = *reinterpret_cast<const uint2*>(l1 + (2 * r + 1) * W1 + cx * 8);
        const uint32_t o = mk_and4(t.x, t.y, b.x, b.y);
        cnt[2] = mk_count(o);
        *reinterpret_cast<uint32_t*>(l2 + r * W2 + cx * 4) = o;
        *reinterpret_cast<uint32_t*>(dst + pa::level_offset(2) + (band * (MK_BAND_ROWS / 4) + r) * W2 + cx * 4) = o;
    }
    __syncthreads();
    if (tid < (MK_BAND_ROWS / 8) * W3) {                                         // 4 rows x 40 level-3 bytes
        const int r = tid / W3, c = tid - r * W3;
        const uint8_t* q = l2 + (2 * r) * W2 + 2 * c;
        const uint8_t o = pm::and4(q[0], q[1], q[W2], q[W2 + 1]);
        cnt[3] = o;
        dst[pa::level_offset(3) + (band * (MK_BAND_ROWS / 8) + r) * W3 + c] = o;
    }
    // (every thread is here: whole waves in the shuffle tree)
#pragma unroll
    for (int L = 0; L < pa::MAX_LEVELS; L++) {
        const int t = wave_sum(cnt[L]);
        if (lane == 0) w_cnt[wave * pa::MAX_LEVELS + L] = t;
    }
    __syncthreads();
    if (tid < pa::MAX_LEVELS) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < MK_WAVES; w++) t += w_cnt[w * pa::MAX_LEVELS + tid];
        n_mask[(size_t)f * N_MASK + tid * PHOTO_SLICES + band] = t;
    }
}

// grid: PHOTO_SLICES * n workgroups of pr_threads(L) (slice = block % PHOTO_SLICES).  photo_robust_accum_kernel<L>'s arguments, and mask: the level-L mask
// of pair 0 (the same stride), n_mask [n][N_MASK].
template <int L>
__global__ __launch_bounds__(pr_threads(L)) void photo_masked_accum_kernel(const uint8_t* __restrict__ img1, const uint8_t* __restrict__ img2,
                                                                           const uint8_t* __restrict__ mask, const int32_t* __restrict__ n_mask, int stride,
                                                                           float kf, const RobustStart* __restrict__ start,
                                                                           const RobustWork* __restrict__ work, const RobustRec* __restrict__ rec,
                                                                           RobustSums* __restrict__ partial) {
    constexpr int W = pa::level_w(L), LPIX = pa::level_pix(L), SLICE_PIX = LPIX / PHOTO_SLICES, THREADS = pr_threads(L), WAVES = THREADS / 64;
    static_assert(L >= 0 && L < pa::MAX_LEVELS && pa::level_h(L) % PHOTO_SLICES == 0 && LPIX % 16 == 0 && pa::level_offset(L) % 16 == 0, "whole rows per slice");
    static_assert(L > 0 || (SLICE_PIX % (4 * THREADS) == 0 && W % 4 == 0), "whole quads per thread at level 0");
    static_assert(sizeof(RobustSums) % 4 == 0, "a partial is whole words");
    extern __shared__ __attribute__((aligned(16))) uint8_t pr_lds[];
    const int pair = blockIdx.x / PHOTO_SLICES, slice = blockIdx.x - pair * PHOTO_SLICES;
    if (!start && rec[pair].px.flags != 0) return;                            // (workgroup-uniform)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    RobustSums* out = partial + (size_t)pair * PHOTO_SLICES + slice;
    if (n_mask[(size_t)pair * N_MASK + L * PHOTO_SLICES + slice] == 0) {      // (workgroup-uniform: nothing of this slice takes part)
        for (int e = tid; e < (int)(sizeof(RobustSums) / 4); e += THREADS) reinterpret_cast<uint32_t*>(out)[e] = 0u;
        return;
    }
    double* w_sum = reinterpret_cast<double*>(pr_lds + LPIX);
    int* w_cnt = reinterpret_cast<int*>(w_sum + WAVES * PR_ND);
    float* hs = reinterpret_cast<float*>(w_cnt + WAVES * 2);
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
    const uint8_t* m_img = mask + (size_t)pair * stride;
    double acc[PR_ND];
#pragma unroll
    for (int k = 0; k < PR_ND; k++) acc[k] = 0.0;
    int n_valid = 0, n_out = 0;
    if constexpr (L == 0) {
        const int pix0 = slice * SLICE_PIX + 4 * tid;
        for (int q = 0; q < SLICE_PIX / (4 * THREADS); q++) {
            const int pix = pix0 + q * (4 * THREADS);
            const int v = pix / W, u0 = pix - v * W;
            const uint32_t a4 = *reinterpret_cast<const uint32_t*>(a_img + pix), m4 = *reinterpret_cast<const uint32_t*>(m_img + pix);
            if (m4 == 0u) continue;
            for (int j = 0; j < 4; j++) {
                pr_pixel<L>(h, Gf, bf, kf, tile, u0 + j, v, PixRead<uint8_t>::cvt((uint8_t)(a4 >> (8 * j))), acc, n_valid, n_out, ((m4 >> (8 * j)) & 0xFFu) != 0u);
            }
        }
    } else {
        for (int i = tid; i < SLICE_PIX; i += THREADS) {
            const int pix = slice * SLICE_PIX + i;
            const int v = pix / W, u = pix - v * W;
            pr_pixel<L>(h, Gf, bf, kf, tile, u, v, PixRead<uint8_t>::cvt(a_img[pix]), acc, n_valid, n_out, m_img[pix] != 0);
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

hipError_t photo_masked_init_device() {
    return hipFuncSetAttribute((const void*)photo_masked_accum_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, pr_lds_bytes(0));
}

hipError_t launch_photo_mask_pyramid(const uint8_t* mask, int n, uint8_t* mpyr, int32_t* n_mask, hipStream_t s) {
    if (n < 1 || n >= (1 << 16) || !mask || !mpyr || !n_mask || (((uintptr_t)mask) & 15) || (((uintptr_t)mpyr) & 15)) return hipErrorInvalidValue;      // (n masks in grid.y)
    hipLaunchKernelGGL(photo_mask_pyramid_kernel, dim3(PHOTO_SLICES, (unsigned)n), dim3(MK_THREADS), 0, s, mask, mpyr, n_mask);
    return hipGetLastError();
}

namespace {
template <int L>
void masked_accum(const uint8_t* img1, const uint8_t* img2, const uint8_t* mask, const int32_t* n_mask, int stride, int n, float kf, const RobustStart* start,
                  const RobustWork* work, const RobustRec* rec, RobustSums* partial, hipStream_t s) {
    hipLaunchKernelGGL(photo_masked_accum_kernel<L>, dim3((unsigned)(n * PHOTO_SLICES)), dim3(pr_threads(L)), pr_lds_bytes(L), s, img1, img2, mask, n_mask, stride, kf,
                       start, work, rec, partial);
}
}  // namespace

void launch_photo_masked_accum(int L, const uint8_t* img1, const uint8_t* img2, const uint8_t* mask, const int32_t* n_mask, int stride, int n, float kf,
                               const RobustStart* start, const RobustWork* work, const RobustRec* rec, RobustSums* partial, hipStream_t s) {
    if (L == 0) masked_accum<0>(img1, img2, mask, n_mask, stride, n, kf, start, work, rec, partial, s);
    else if (L == 1) masked_accum<1>(img1, img2, mask, n_mask, stride, n, kf, start, work, rec, partial, s);
    else if (L == 2) masked_accum<2>(img1, img2, mask, n_mask, stride, n, kf, start, work, rec, partial, s);
    else masked_accum<3>(img1, img2, mask, n_mask, stride, n, kf, start, work, rec, partial, s);
}

}  // namespace hnet
