// photo_align_dev.h — photometric alignment (include/hnet.h hnet_photo_align): what the host code and kernels_photo_align.hip share
// (the launch sequences: photo_pyramid_dev.h for the plain form, photo_robust_dev.h for the gain / bias + Huber form).
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

constexpr int PA_ND = hnet_align::NSYM + hnet_align::NH + 1;      // 55 double sums: ss | sr | rr, the order of AlignSums
// H = (float) dlt_solve(p4 + x) as photo_slice_body forms it; false (and NaN entries) when an entry is not finite
__device__ __forceinline__ bool pa_homography(const float* x, float* h) {
    double d[8], hd[9];
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = hnet_align::corner(p4(k), x[k]);
    dlt_solve(d, hd);
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; k++) ok = ok && isfinite((float)hd[k]);
#pragma unroll
    for (int k = 0; k < 9; k++) h[k] = ok ? (float)hd[k] : __builtin_nanf("");
    return ok;
}

hipError_t photo_align_init_device();      // dynamic-LDS limit of the level-0 accumulate kernels (plain and robust); once per device

}  // namespace hnet
