// photo_robust_dev.h — photometric alignment with a gain / bias model and Huber weights (include/hnet.h hnet_op_photo_align_robust): what the
// host code and kernels_photo_align.hip share.  The device compiles include/hnet_photo_robust.h itself (host + device functions): the residual, the
// weights, the reduction to the ten parameters and the Levenberg-Marquardt step are the functions tests/test_photo_robust_cpu.py pins on the host.
#pragma once
#include "photo_pyramid_dev.h"

#pragma clang force_cuda_host_device begin
#include "../../include/hnet_photo_robust.h"
#pragma clang force_cuda_host_device end

namespace hnet {

using RobustSums = hnet_robust::Sums;        // one linearisation; also one row slice's partial
using RobustRec = hnet_robust::Record;       // = hnet_photo_robust
using RobustWork = hnet_robust::Work;
using RobustOpts = hnet_robust::Opts;        // = hnet_photo_robust_opts
using RobustStart = hnet_robust::Start;
static_assert(sizeof(RobustSums) == 632 && sizeof(RobustRec) == 1560 && sizeof(RobustWork) == 128 && sizeof(RobustOpts) == 56 && sizeof(RobustStart) == 48,
              "packed layouts");

// The whole launch sequence of one call with 1 <= levels <= 4 (the level driver of kernels_photo_align.hip): the pyramid (levels > 1, launch_photo_pyramid),
// then per level from levels - 1 down to 0 one gather of the level's start and max_iterations + 1 pairs of {photo_robust_accum_kernel<L>,
// photo_robust_solve_kernel}.  img1 / img2: device u8 [n][NPIX],
// 16-byte aligned; x0: device float [n][8]; pyr1 / pyr2: [n][PYR_BYTES] of scratch (unused at levels == 1); start, work: [n] of scratch; partial:
// n * PHOTO_SLICES of scratch; rec: [levels][n], rec + L n the records of level L, complete after the last launch.
hipError_t launch_photo_align_robust(const uint8_t* img1, const uint8_t* img2, int n, const float* x0, const RobustOpts& opts, int levels, uint8_t* pyr1,
                                     uint8_t* pyr2, RobustStart* start, RobustSums* partial, RobustWork* work, RobustRec* rec, hipStream_t s);

}  // namespace hnet
