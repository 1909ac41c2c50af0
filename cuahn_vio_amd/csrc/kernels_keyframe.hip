// kernels_keyframe.hip — the device side of tracking against a held keyframe (include/hnet.h hnet_sessions_keyframe_track) around the
// unchanged launch_photo_align_robust: the start of each slot's alignment composed from the session's state, the keyframe and the current frame gathered
// into the staging arrays, the rule of include/hnet_keyframe.h on the level-0 record, and the copy of a new keyframe into the store.  The two per-slot
// kernels are one wavefront each, fp64 on lane 0 with everything in registers, and like kernels_filters_refine.hip built with -ffp-contract=off: compose
// and decide are the host reference's operations in its order.  The two copy kernels move 16-byte vectors, one per lane, like session_gather_kernel.
// No atomics, no LDS, nothing waits on another workgroup.  The host side that enqueues these kernels is capi_keyframe.hip.
#include "keyframe_dev.h"

namespace hnet {

namespace kf = hnet_keyframe;

namespace {
constexpr int SV = NPIX / 16;                       // 16-byte vectors per frame
static_assert(NPIX % 16 == 0, "frames must stay 16-byte aligned in the store, the ring and the staging arrays");
constexpr int SV_BLOCKS = (SV + 255) / 256;
constexpr int REC_DOUBLES = (int)(sizeof(RobustRec) / sizeof(double));
static_assert(sizeof(RobustRec) % sizeof(double) == 0 && offsetof(KeyTrack, rec) == 0, "KeyTrack: the record first, as doubles");
}  // namespace

__global__ __launch_bounds__(KEY_THREADS) void keyframe_start_kernel(KeyTable tab, int n, int n_sessions, const KeyState* __restrict__ state, float* __restrict__ x0) {
    const int b = blockIdx.x;
    if (b >= n || threadIdx.x != 0) return;
    const int id = tab.ids[b];
    float* o = x0 + (size_t)b * 8;
    bool ok = id >= 0 && id < n_sessions && state[id].has_key != 0;
    if (ok) ok = kf::compose(tab.step + (size_t)b * 8, state[id].key_px, o);
    if (!ok)
        for (int k = 0; k < 8; k++) o[k] = kf::quiet_nan();
}

__global__ __launch_bounds__(256) void keyframe_gather_kernel(KeyTable tab, int n_sessions, const uint4* __restrict__ key, const uint4* __restrict__ ring, int n_slots,
                                                              uint4* __restrict__ prev, uint4* __restrict__ curr) {
    const int v = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    const int id = tab.ids[b], sc = tab.slot[b];
    if (v >= SV || id < 0 || id >= n_sessions || sc < 0 || sc >= n_slots) return;
    const uint4 p = key[(size_t)id * SV + v], c = ring[(size_t)sc * SV + v];
    prev[(size_t)b * SV + v] = p;
    curr[(size_t)b * SV + v] = c;
}

__global__ __launch_bounds__(KEY_THREADS) void keyframe_decide_kernel(KeyTable tab, int n, int n_sessions, const RobustRec* __restrict__ rec, const float* x0, KeyOpts opts,
                                                                      KeyState* state, KeyTrack* out, int32_t* __restrict__ copy) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return;
    const int id = tab.ids[b];
    const bool valid = id >= 0 && id < n_sessions;                               // (uniform over the workgroup)
    const bool read = valid && state[id].has_key != 0;                           // (read by every lane before lane 0 writes the state: one wavefront, in order)
    const double* src = reinterpret_cast<const double*>(rec + b);
    double* dst = reinterpret_cast<double*>(out + b);
    for (int i = t; i < REC_DOUBLES; i += KEY_THREADS) dst[i] = read ? src[i] : 0.0;
    if (t != 0) return;
    if (!valid) {
        for (int i = REC_DOUBLES; i < (int)(sizeof(KeyTrack) / sizeof(double)); i++) dst[i] = 0.0;
        copy[b] = 0;
        return;
    }
    copy[b] = kf::decide(state[id], x0 + (size_t)b * 8, rec[b], opts, tab.gap[b] != 0, state[id], out[b]);
}

__global__ __launch_bounds__(256) void keyframe_commit_kernel(KeyTable tab, int n_sessions, const int32_t* __restrict__ copy, const uint4* __restrict__ curr,
                                                              uint4* __restrict__ key) {
    const int v = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (copy[b] == 0) return;
    const int id = tab.ids[b];
    if (v >= SV || id < 0 || id >= n_sessions) return;
    key[(size_t)id * SV + v] = curr[(size_t)b * SV + v];
}

hipError_t launch_keyframe_start(const KeyTable& tab, int n, int n_sessions, const KeyState* state, float* x0, hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyframe_start_kernel, dim3((unsigned)n), dim3(KEY_THREADS), 0, s, tab, n, n_sessions, state, x0);
    return hipGetLastError();
}

hipError_t launch_keyframe_gather(const KeyTable& tab, int n, int n_sessions, const uint8_t* key, const uint8_t* ring, int n_slots, uint8_t* prev, uint8_t* curr,
                                  hipStream_t s) {
    if (n < 1 || n > 65535 || ((((uintptr_t)key) | (uintptr_t)ring | (uintptr_t)prev | (uintptr_t)curr) & 15)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyframe_gather_kernel, dim3(SV_BLOCKS, (unsigned)n), dim3(256), 0, s, tab, n_sessions, (const uint4*)key, (const uint4*)ring, n_slots,
                       (uint4*)prev, (uint4*)curr);
    return hipGetLastError();
}

hipError_t launch_keyframe_decide(const KeyTable& tab, int n, int n_sessions, const RobustRec* rec, const float* x0, const KeyOpts& opts, KeyState* state,
                                  KeyTrack* out, int32_t* copy, hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyframe_decide_kernel, dim3((unsigned)n), dim3(KEY_THREADS), 0, s, tab, n, n_sessions, rec, x0, opts, state, out, copy);
    return hipGetLastError();
}

hipError_t launch_keyframe_commit(const KeyTable& tab, int n, int n_sessions, const int32_t* copy, const uint8_t* curr, uint8_t* key, hipStream_t s) {
    if (n < 1 || n > 65535 || ((((uintptr_t)key) | (uintptr_t)curr) & 15)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyframe_commit_kernel, dim3(SV_BLOCKS, (unsigned)n), dim3(256), 0, s, tab, n_sessions, copy, (const uint4*)curr, (uint4*)key);
    return hipGetLastError();
}

}  // namespace hnet
