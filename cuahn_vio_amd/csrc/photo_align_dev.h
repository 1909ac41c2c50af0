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

// what the accumulate kernels of every level share (kernels_photo_align.hip: level 0; kernels_photo_pyramid.hip: the coarse levels)
constexpr int PA_ND = hnet_align::NSYM + hnet_align::NH + 1;      // 55 double sums: ss | sr | rr, the order of AlignSums
__device__ __forceinline__ double pa_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    return v;
}
__device__ __forceinline__ int pa_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    return v;
}
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

hipError_t photo_align_init_device();      // dynamic-LDS limit of photo_align_accum_kernel; once per device
// The whole launch sequence of one call: max_iterations + 1 pairs of {photo_align_accum_kernel, photo_align_solve_kernel} on stream s, nothing else.
// img1 / img2: device u8 [n][NPIX], 16-byte aligned; x0: device float [n][8]; partial: n * PHOTO_SLICES sums of scratch; work: [n] of scratch;
// rec: [n], written by the first solve launch and complete after the last.
hipError_t launch_photo_align(const uint8_t* img1, const uint8_t* img2, int n, const float* x0, const AlignOpts& opts, AlignSums* partial, AlignWork* work,
                              AlignRec* rec, hipStream_t s);

// one launch of photo_align_solve_kernel: linearisation `it` of n pairs, whose 7 slice partials any accumulate kernel left in partial (the coarse levels of
// photo_pyramid_dev.h run on it unchanged)
hipError_t launch_photo_align_solve(const AlignSums* partial, const float* x0, int it, const AlignOpts& opts, int n, AlignWork* work, AlignRec* rec, hipStream_t s);

}  // namespace hnet
