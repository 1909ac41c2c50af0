// kernels_keyframe_localise.hip — the small kernels of a localise against a rendered keyframe map (keyframe_localise_dev.h, include/hnet.h
// hnet_op_keyframe_localise), around the UNCHANGED render (kernels_keyframe_render.hip) and the masked alignment (kernels_photo_masked.hip,
// kernels_photo_align.hip): the start of the alignment from the render's record, and the verdict.  The rule is include/hnet_keyframe_localise.h's, compiled
// here without contraction like every keyframe kernel.
#include "keyframe_localise_dev.h"

namespace hnet {

namespace kl = hnet_localise;

// grid: ceil(n / 64) workgroups of 64; one thread per slot
__global__ __launch_bounds__(64) void keyframe_localise_start_kernel(const RenderRec* __restrict__ rrec, int n, LocaliseOpts opts, float* __restrict__ x0) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n) return;
    float x[8];
    kl::start(rrec[b].used_mask, rrec[b].c.n_covered, opts, x);
#pragma unroll
    for (int k = 0; k < 8; k++) x0[(size_t)b * 8 + k] = x[k];
}

// grid: ceil(n / 64) workgroups of 64; one thread per slot
__global__ __launch_bounds__(64) void keyframe_localise_eligible_kernel(const int32_t* __restrict__ ids, int n, MapStore map, RenderTab* tab, RenderRec* rrec) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n) return;
    const int id = ids[b];
    if (id < 0 || id >= map.n_sessions || map.capacity < 1 || map.capacity > RENDER_MAX) return;      // (the render's setup left an empty mask)
    const MapState m = map.state[id];
    const int used = tab[b].used_mask & kl::eligible_mask(&m, map.entry + (size_t)id * map.capacity, map.capacity);
    tab[b].used_mask = used;
    rrec[b].used_mask = used;
}

// grid: (NPIX / 16 / 256, n) workgroups of 256: a uint4 per lane; lane 0 of the first workgroup of a slot writes its start
__global__ __launch_bounds__(256) void keyframe_localise_gather_kernel(const int32_t* __restrict__ slot, const uint8_t* __restrict__ ring, int n_slots,
                                                                       const RenderRec* __restrict__ rrec, LocaliseOpts opts, uint8_t* __restrict__ curr,
                                                                       float* __restrict__ x0) {
    const int b = blockIdx.y, v = blockIdx.x * 256 + threadIdx.x, sl = slot[b];
    const bool ok = sl >= 0 && sl < n_slots;                                      // (uniform over the workgroup)
    if (ok && v < NPIX / 16) reinterpret_cast<uint4*>(curr + (size_t)b * NPIX)[v] = reinterpret_cast<const uint4*>(ring + (size_t)sl * NPIX)[v];
    if (v == 0) {
        float x[8];
        kl::start(ok ? rrec[b].used_mask : 0, rrec[b].c.n_covered, opts, x);
#pragma unroll
        for (int k = 0; k < 8; k++) x0[(size_t)b * 8 + k] = x[k];
    }
}

// grid: n workgroups of 64
__global__ __launch_bounds__(64) void keyframe_localise_decide_kernel(const int32_t* __restrict__ ids, const RenderRec* __restrict__ rrec,
                                                                      const RobustRec* __restrict__ arec, KeyState* state, MapStore map, LocaliseOpts opts,
                                                                      LocaliseRec* out) {
    static_assert(sizeof(RobustRec) % 4 == 0 && offsetof(LocaliseRec, rec) == 0, "the alignment record leads the localise record, in whole words");
    const int b = blockIdx.x, tid = threadIdx.x;
    const RenderRec& r = rrec[b];
    const bool aligned = kl::covered(r.used_mask, r.c.n_covered, opts);            // (uniform over the workgroup)
    const uint32_t* src = reinterpret_cast<const uint32_t*>(arec + b);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&out[b].rec);
    for (int e = tid; e < (int)(sizeof(RobustRec) / 4); e += 64) dst[e] = aligned ? src[e] : 0u;
    __syncthreads();
    if (tid != 0) return;
    const int id = ids ? ids[b] : -1;
    if (ids && id >= 0 && id < map.n_sessions) {
        MapEntry* e = map.entry + (size_t)id * map.capacity;
        kl::decide_localise(state + id, map.state + id, e, map.capacity, r.used_mask, r.c.n_covered, r.h_origin_view, out[b].rec, opts, state + id, map.state + id, e,
                            out[b]);
    } else {
        kl::decide_localise(nullptr, nullptr, ids ? nullptr : map.entry + (size_t)b * map.capacity, ids ? 0 : map.capacity, ids ? 0 : r.used_mask, r.c.n_covered,
                            r.h_origin_view, out[b].rec, opts, nullptr, nullptr, nullptr, out[b]);
    }
}

hipError_t launch_keyframe_localise_start(const RenderRec* rrec, int n, const LocaliseOpts& opts, float* x0, hipStream_t s) {
    if (!rrec || !x0 || n < 1 || !kl::opts_valid(opts)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyframe_localise_start_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, rrec, n, opts, x0);
    return hipGetLastError();
}

hipError_t launch_keyframe_localise_eligible(const int32_t* ids, int n, const MapStore& map, RenderTab* tab, RenderRec* rrec, hipStream_t s) {
    if (!ids || !tab || !rrec || !map.entry || !map.state || n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyframe_localise_eligible_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, ids, n, map, tab, rrec);
    return hipGetLastError();
}

hipError_t launch_keyframe_localise_gather(const int32_t* slot, int n, const uint8_t* ring, int n_slots, const RenderRec* rrec, const LocaliseOpts& opts,
                                           uint8_t* curr, float* x0, hipStream_t s) {
    if (!slot || !ring || !rrec || !curr || !x0 || n < 1 || n > 65535 || n_slots < 1 || !kl::opts_valid(opts) || (((uintptr_t)ring | (uintptr_t)curr) & 15))
        return hipErrorInvalidValue;
    static_assert(NPIX % 16 == 0, "whole uint4 per frame");
    hipLaunchKernelGGL(keyframe_localise_gather_kernel, dim3((unsigned)((NPIX / 16 + 255) / 256), (unsigned)n), dim3(256), 0, s, slot, ring, n_slots, rrec, opts, curr, x0);
    return hipGetLastError();
}

hipError_t launch_keyframe_localise_decide(const int32_t* ids, int n, const RenderRec* rrec, const RobustRec* arec, KeyState* state, const MapStore& map,
                                           const LocaliseOpts& opts, LocaliseRec* out, hipStream_t s) {
    if (!rrec || !arec || !map.entry || !out || n < 1 || map.capacity < 1 || map.capacity > RENDER_MAX || !kl::opts_valid(opts)) return hipErrorInvalidValue;
    if (ids && (!state || !map.state)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyframe_localise_decide_kernel, dim3((unsigned)n), dim3(64), 0, s, ids, rrec, arec, state, map, opts, out);
    return hipGetLastError();
}

}  // namespace hnet
