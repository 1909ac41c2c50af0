// kernels_sessions.hip — the device side of hnet_sessions (include/hnet.h): many camera streams on one context.
// A sessions object keeps a device ring of n_sessions x 2 frames of 224 x 320 u8 (slot 2 id + k); these kernels move frames between that ring, the staging
// slabs a push uploads and the contiguous prev / curr arrays the unchanged forward reads.  Every frame is NPIX = 71 680 bytes = 4 480 16-byte vectors and every
// frame base is 16-byte aligned (hipMalloc'd bases, NPIX a multiple of 16), so the forward's tiled prep kernels (prep_fc_supported) and the copies below
// see aligned frames.  Slot indices come from host-validated tables; the kernels still skip a slot outside the ring instead of writing past it.
#include "kernels.h"
#include "geom.h"
#include "undistort_dev.h"

namespace hnet {

namespace {
constexpr int SV = NPIX / 16;                       // 16-byte vectors per frame
static_assert(NPIX % 16 == 0, "frames must stay 16-byte aligned in the ring and the staging arrays");
constexpr int SV_BLOCKS = (SV + 255) / 256;        // 18 workgroups of 256 threads per frame
}  // namespace

// frame i of the staged slab [n][NPIX] -> ring slot dst_slot[i]; grid (SV_BLOCKS, n)
__global__ __launch_bounds__(256) void session_scatter_kernel(const uint4* __restrict__ staged, const int32_t* __restrict__ dst_slot, int n_slots,
                                                              uint4* __restrict__ ring) {
    const int v = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    const int slot = dst_slot[i];
    if (v >= SV || slot < 0 || slot >= n_slots) return;
    ring[(size_t)slot * SV + v] = staged[(size_t)i * SV + v];
}

// pair b: prev[b] <- ring slot pair_slot[2 b], curr[b] <- ring slot pair_slot[2 b + 1]; grid (SV_BLOCKS, n)
__global__ __launch_bounds__(256) void session_gather_kernel(const uint4* __restrict__ ring, int n_slots, const int32_t* __restrict__ pair_slot,
                                                             uint4* __restrict__ prev, uint4* __restrict__ curr) {
    const int v = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    const int sp = pair_slot[2 * b], sc = pair_slot[2 * b + 1];
    if (v >= SV || sp < 0 || sp >= n_slots || sc < 0 || sc >= n_slots) return;
    const uint4 p = ring[(size_t)sp * SV + v], c = ring[(size_t)sc * SV + v];
    prev[(size_t)b * SV + v] = p;
    curr[(size_t)b * SV + v] = c;
}

// frame i: raw image i of the slab (raw_frame bytes apart, rows x cols, packed rows) remapped with the maps of camera cam[i] (maps[2 cam] = x, [2 cam + 1] = y)
// straight into ring slot dst_slot[i]; one output pixel per thread (undistort_pixel: the bits of undistort_kernel); grid ((NPIX + 255) / 256, n)
__global__ __launch_bounds__(256) void session_remap_kernel(const uint8_t* __restrict__ raw, size_t raw_frame, int rows, int cols,
                                                            const int32_t* __restrict__ dst_slot, const int32_t* __restrict__ cam,
                                                            const float* const* __restrict__ maps, int n_cams, int n_slots, uint8_t* __restrict__ ring) {
    const int p = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    const int slot = dst_slot[i], k = cam[i];
    if (p >= NPIX || slot < 0 || slot >= n_slots || k < 0 || k >= n_cams) return;
    ring[(size_t)slot * NPIX + p] = undistort_pixel(raw + (size_t)i * raw_frame, rows, cols, cols, maps[2 * k], maps[2 * k + 1], p);
}

hipError_t launch_session_scatter(const uint8_t* staged, const int32_t* dst_slot, int n, int n_slots, uint8_t* ring, hipStream_t s) {
    if (n < 1 || n > 65535 || ((((uintptr_t)staged) | (uintptr_t)ring) & 15)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(session_scatter_kernel, dim3(SV_BLOCKS, (unsigned)n), dim3(256), 0, s, (const uint4*)staged, dst_slot, n_slots, (uint4*)ring);
    return hipGetLastError();
}

hipError_t launch_session_gather(const uint8_t* ring, int n_slots, const int32_t* pair_slot, int n, uint8_t* prev, uint8_t* curr, hipStream_t s) {
    if (n < 1 || n > 65535 || ((((uintptr_t)ring) | (uintptr_t)prev | (uintptr_t)curr) & 15)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(session_gather_kernel, dim3(SV_BLOCKS, (unsigned)n), dim3(256), 0, s, (const uint4*)ring, n_slots, pair_slot, (uint4*)prev, (uint4*)curr);
    return hipGetLastError();
}

hipError_t launch_session_remap(const uint8_t* raw, size_t raw_frame, int rows, int cols, const int32_t* dst_slot, const int32_t* cam, const float* const* maps,
                                int n_cams, int n, int n_slots, uint8_t* ring, hipStream_t s) {
    if (n < 1 || n > 65535 || rows < 1 || cols < 1 || raw_frame < (size_t)rows * cols) return hipErrorInvalidValue;
    hipLaunchKernelGGL(session_remap_kernel, dim3((NPIX + 255) / 256, (unsigned)n), dim3(256), 0, s, raw, raw_frame, rows, cols, dst_slot, cam, maps, n_cams,
                       n_slots, ring);
    return hipGetLastError();
}

}  // namespace hnet
