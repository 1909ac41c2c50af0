// undistort_dev.h — one output pixel of the undistort + resize remap (CamBase::undistort_and_resize_img = cv::remap(INTER_LINEAR, BORDER_CONSTANT 0),
// CamBase.h:182-186), shared by undistort_kernel (kernels.hip, one frame) and session_remap_kernel (kernels_sessions.hip, one frame per session): same bits.
// out(v, u) = bilinear(raw, map_x(v, u), map_y(v, u)).  Sample positions are quantised to 1/32 px as cv::remap does (INTER_BITS = 5, round half to even),
// the blend is exact integer arithmetic: weights (32-ax)(32-ay) ... sum 1024, result (sum + 512) >> 10.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hnet {

// i: output pixel (row-major 224 x 320); raw: rows x cols bytes, `stride` bytes per row
__device__ __forceinline__ uint8_t undistort_pixel(const uint8_t* __restrict__ raw, int rows, int cols, int stride, const float* __restrict__ map_x,
                                                   const float* __restrict__ map_y, int i) {
    const float fx = map_x[i] * 32.0f, fy = map_y[i] * 32.0f;
    // saturate like cv::saturate_cast<short> of the integer part does, and keep NaN / huge positions out of the image
    const bool sane = fabsf(fx) < 1.0e9f && fabsf(fy) < 1.0e9f;
    const int sx = sane ? __float2int_rn(fx) : -(1 << 20), sy = sane ? __float2int_rn(fy) : -(1 << 20);
    const int x0 = sx >> 5, y0 = sy >> 5, ax = sx & 31, ay = sy & 31;
    auto tap = [&](int y, int x) -> int { return ((unsigned)y < (unsigned)rows && (unsigned)x < (unsigned)cols) ? (int)raw[(size_t)y * stride + x] : 0; };
    const int v = tap(y0, x0) * (32 - ax) * (32 - ay) + tap(y0, x0 + 1) * ax * (32 - ay) + tap(y0 + 1, x0) * (32 - ax) * ay +
                  tap(y0 + 1, x0 + 1) * ax * ay;
    return (uint8_t)((v + 512) >> 10);
}

}  // namespace hnet
