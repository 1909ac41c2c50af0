// kernels_photo_pyramid.hip — the image pyramid of photometric alignment (photo_pyramid_dev.h, include/hnet.h hnet_op_photo_pyramid).  The
// alignment on its levels is kernels_photo_align.hip's.
//
// photo_pyramid_kernel: ONE launch per call makes levels 1, 2, 3 of every frame.  A workgroup of 320 threads owns a band of 32 rows of one frame: each thread
// reads 16 pixels of two adjacent rows with two 16-byte loads (level 0 is read once), writes its 8 level-1 pixels to global memory and to LDS; level 2 is
// made from the ROUNDED level 1 in LDS, level 3 from level 2 in LDS (hnet_align::down4: exact integers, bit-identical to the host reference).
#include "photo_pyramid_dev.h"

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

hipError_t launch_photo_pyramid(const uint8_t* img_a, const uint8_t* img_b, int n, uint8_t* pyr_a, uint8_t* pyr_b, hipStream_t s) {
    if (n < 1 || n >= (1 << 15) || !img_a || !pyr_a || (img_b != nullptr) != (pyr_b != nullptr)) return hipErrorInvalidValue;      // (2 n frames in grid.y)
    if ((((uintptr_t)img_a) & 15) || (((uintptr_t)img_b) & 15) || (((uintptr_t)pyr_a) & 15) || (((uintptr_t)pyr_b) & 15)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(photo_pyramid_kernel, dim3(PYR_BANDS, (unsigned)(img_b ? 2 * n : n)), dim3(PYR_THREADS), 0, s, img_a, img_b, n, pyr_a, pyr_b);
    return hipGetLastError();
}

}  // namespace hnet
