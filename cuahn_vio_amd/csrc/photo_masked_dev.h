// photo_masked_dev.h — the robust photometric alignment on the template pixels a mask admits (include/hnet.h hnet_op_photo_align_masked): what
// the host code, kernels_photo_masked.hip (the mask pyramid and the accumulate kernels) and kernels_photo_align.hip (the level driver) share.  The device
// compiles include/hnet_photo_masked.h itself (host + device functions): the AND rule of the mask pyramid is the function tests/test_photo_masked_cpu.py pins
// on the host.
#pragma once
#include "photo_robust_dev.h"

#pragma clang force_cuda_host_device begin
#include "../../include/hnet_photo_masked.h"
#pragma clang force_cuda_host_device end

namespace hnet {

constexpr int N_MASK = hnet_masked::N_MASK;      // counts of one mask: [level 0 .. 3][slice 0 .. 6]
static_assert(hnet_masked::SLICES == PHOTO_SLICES, "the counts are per slice of an accumulate launch");

hipError_t photo_masked_init_device();      // dynamic-LDS limit of the level-0 masked accumulate kernel; once per device

// levels 1 .. 3 of n masks and the counts of all four levels, ONE launch: mask device u8 [n][NPIX], 16-byte aligned -> mpyr [n][PYR_BYTES] (bytes 0 / 1),
// n_mask [n][N_MASK]
hipError_t launch_photo_mask_pyramid(const uint8_t* mask, int n, uint8_t* mpyr, int32_t* n_mask, hipStream_t s);

// One accumulate launch of level L (0 .. 3) for the level driver: photo_robust_accum_kernel<L>'s arguments (img1 / img2 / mask: the level-L arrays of pair 0,
// `stride` bytes from a pair to the next) and n_mask [n][N_MASK].  Errors are left to hipGetLastError.
void launch_photo_masked_accum(int L, const uint8_t* img1, const uint8_t* img2, const uint8_t* mask, const int32_t* n_mask, int stride, int n, float kf,
                               const RobustStart* start, const RobustWork* work, const RobustRec* rec, RobustSums* partial, hipStream_t s);

// launch_photo_align_robust (photo_robust_dev.h) with a mask beside img1: the mask pyramid, then the same launch sequence with photo_masked_accum_kernel<L>
// in the place of photo_robust_accum_kernel<L>.  mask1: device u8 [n][NPIX], 16-byte aligned; mpyr: [n][PYR_BYTES] and n_mask: [n][N_MASK] of scratch (both
// used at every `levels`).
hipError_t launch_photo_align_masked(const uint8_t* img1, const uint8_t* mask1, const uint8_t* img2, int n, const float* x0, const RobustOpts& opts, int levels,
                                     uint8_t* pyr1, uint8_t* pyr2, uint8_t* mpyr, int32_t* n_mask, RobustStart* start, RobustSums* partial, RobustWork* work,
                                     RobustRec* rec, hipStream_t s);

}  // namespace hnet
