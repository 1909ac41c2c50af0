// photo_align_dev.h — photometric alignment (include/hnet.h hnet_photo_align): what the host code and kernels_photo_align.hip share.
// The device compiles include/hnet_photo_align.h itself (host + device functions): the Jacobian of the DLT, the reduction to the offsets and the
// Levenberg-Marquardt step are the functions tests/test_photo_align_cpu.py pins on the host.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#pragma clang force_cuda_host_device begin
#include "../../include/hnet_photo_align.h"
#pragma clang force_cuda_host_device end

#include "photo_dev.h"

namespace hnet {

using AlignSums = hnet_align::Sums;          // one linearisation in H-space; also one row slice's partial
using AlignRec = hnet_align::Record;         // = hnet_photo_align
using AlignWork = hnet_align::Work;
using AlignOpts = hnet_align::Opts;
static_assert(sizeof(AlignSums) == 448 && sizeof(AlignRec) == 656 && sizeof(AlignWork) == 96, "packed layouts");

hipError_t photo_align_init_device();      // dynamic-LDS limit of photo_align_accum_kernel; once per device
// The whole launch sequence of one call: max_iterations + 1 pairs of {photo_align_accum_kernel, photo_align_solve_kernel} on stream s, nothing else.
// img1 / img2: device u8 [n][NPIX], 16-byte aligned; x0: device float [n][8]; partial: n * PHOTO_SLICES sums of scratch; work: [n] of scratch;
// rec: [n], written by the first solve launch and complete after the last.
hipError_t launch_photo_align(const uint8_t* img1, const uint8_t* img2, int n, const float* x0, const AlignOpts& opts, AlignSums* partial, AlignWork* work,
                              AlignRec* rec, hipStream_t s);

}  // namespace hnet
