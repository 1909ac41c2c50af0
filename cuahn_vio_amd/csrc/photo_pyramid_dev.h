// photo_pyramid_dev.h — coarse-to-fine photometric alignment (include/hnet.h hnet_op_photo_align_pyramid): what the host code,
// kernels_photo_pyramid.hip (the pyramid) and kernels_photo_align.hip (the alignment on it) share.  The device compiles include/hnet_photo_pyramid.h itself (host + device functions): the down-sampling rule, the level
// geometry and the per-pixel quantity of a level are the functions tests/test_photo_align_pyr_cpu.py pins on the host.
#pragma once
#include "photo_align_dev.h"

#pragma clang force_cuda_host_device begin
#include "../../include/hnet_photo_pyramid.h"
#pragma clang force_cuda_host_device end

namespace hnet {

constexpr int PYR_BYTES = hnet_align::PYR_BYTES;      // levels 1 .. 3 of one frame, packed
static_assert(hnet_align::PYR_W0 == IMG_W && hnet_align::PYR_H0 == IMG_H, "level 0 is the network's frame");

// levels 1 .. 3 of n frames (and of n more when img_b != nullptr), ONE launch: img_* device u8 [n][NPIX], 16-byte aligned -> pyr_* [n][PYR_BYTES]
hipError_t launch_photo_pyramid(const uint8_t* img_a, const uint8_t* img_b, int n, uint8_t* pyr_a, uint8_t* pyr_b, hipStream_t s);

// The whole launch sequence of one call with 1 <= levels <= 4 (kernels_photo_align.hip, the level driver): the pyramid (levels > 1), then per level from
// levels - 1 down to 0 a gather of the start offsets (below the coarsest) and max_iterations + 1 pairs of {photo_align_accum_kernel or photo_pyr_accum_kernel<L>,
// photo_align_solve_kernel}; levels == 1 is those pairs at x0 and nothing else.  img1 / img2: device u8 [n][NPIX], 16-byte aligned; x0: device float [n][8];
// pyr1 / pyr2: [n][PYR_BYTES] of scratch and start: float [n][8] of scratch (all three unused at levels == 1); partial: n * PHOTO_SLICES sums of scratch;
// work: [n] of scratch; rec: [levels][n], rec + L n the records of level L, complete after the last launch.
hipError_t launch_photo_align_pyramid(const uint8_t* img1, const uint8_t* img2, int n, const float* x0, const AlignOpts& opts, int levels, uint8_t* pyr1,
                                      uint8_t* pyr2, float* start, AlignSums* partial, AlignWork* work, AlignRec* rec, hipStream_t s);

}  // namespace hnet
