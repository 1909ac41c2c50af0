// photo_dev.h — photometric residual records (include/hnet.h hnet_photo_residual): what the host code and kernels_photo.hip share.
// One record per (frame pair, candidate four-corner offset vector): the sum of the reference's error map |warp(img2, H) - img1| * 255
// (model_to_trace.py:319-327) for H = (float) dlt_solve(p4 + offsets), over all pixels and over the pixels that sample inside img2.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "geom.h"

namespace hnet {

constexpr int PHOTO_MAX_CAND = 66;                        // candidates per pair (the filters' 2 + max_iekf_iteration, at most 2 + 64)
// a pair is cut into row slices, one workgroup each; the slice count is a constant so that a pair's record depends on nothing but the pair
constexpr int PHOTO_SLICES = 7;
constexpr int PHOTO_SLICE_PIX = NPIX / PHOTO_SLICES;      // 32 rows = 10 240 pixels = 10 quads of 4 pixels per thread of a 256-thread workgroup
static_assert(IMG_H % PHOTO_SLICES == 0 && PHOTO_SLICE_PIX % (4 * 256) == 0 && IMG_W % 4 == 0, "whole rows per slice, whole quads per thread");
constexpr int PHOTO_DEGENERATE = 1;                       // flags: H has a non-finite entry
constexpr int PHOTO_REJECTED = 2;                         // flags: the photometric gate refused this estimate (photo_gate_kernel)

struct PhotoRec { double sum, sum_inside; int32_t n_inside, flags; };       // = hnet_photo_residual; also one slice's partial
static_assert(sizeof(PhotoRec) == 24, "records are 24 bytes");

// where the kernel finds candidate c of pair b:
//   offsets != nullptr: offsets[(b m + c) 8 ..]                                              (operator / sessions call)
//   offsets == nullptr (a filters step): c = 0 zero offsets, c = 1 prior[b 8 ..], c >= 2 net[(c - 2) net_iter_stride + b 72 ..] (the packed mean of forward c - 2)
struct PhotoCands { const float* offsets; const float* prior; const float* net; size_t net_iter_stride; };

// one fixed tree over the 64 lanes; the total ends in lane 0 (the residual records and every accumulate kernel of the alignment reduce with it)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    return v;
}

inline size_t photo_partial_count(int n, int m) { return (size_t)n * m * PHOTO_SLICES; }      // PhotoRec partials launch_photo_residual needs

hipError_t photo_init_device();       // dynamic-LDS limit of photo_residual_kernel; once per device
// img1 / img2: device u8 [n][NPIX], 16-byte aligned; partial: photo_partial_count(n, m) records of scratch; out: [n][m]; map: nullptr or float [n][m][NPIX]
hipError_t launch_photo_residual(const uint8_t* img1, const uint8_t* img2, int n, const PhotoCands& cands, int m, PhotoRec* partial, PhotoRec* out, float* map,
                                 hipStream_t s);


// ---- the photometric gate of the filters (hnet_filters_set_photo_gate): the records per iteration, in front of the update they guard.
struct PhotoGate { double max_ratio; int32_t min_inside, pad; };            // one session's gate; max_ratio 0 = none
// Iteration `it` of a step of n pairs with `iters` iterations: the slice partials of its candidates ({zero, prior, forward 0} at it == 0, {forward it} later;
// cands as a filters step's, offsets null) into partial [n][2 + iters][PHOTO_SLICES], then photo_gate_kernel: the finished records into rec [n][2 + iters]
// and the verdict of hnet_ekf::photo_reject per slot (gates [n_sessions] by ids[b]; gate / updates [n] as the step's; verdict [n], written for every slot at
// it == 0).  staged (iterations past 0; the three candidates of iteration 0 always share a staged img2): img2 through LDS, else taps from global memory;
// the records' bits do not depend on it.
hipError_t launch_photo_iteration(const uint8_t* img1, const uint8_t* img2, int n, const PhotoCands& cands, int it, int iters, bool staged, PhotoRec* partial,
                                  const int32_t* ids, int n_sessions, const PhotoGate* gates, const int32_t* updates, int32_t* gate, int32_t* verdict, PhotoRec* rec,
                                  hipStream_t s);

}  // namespace hnet
