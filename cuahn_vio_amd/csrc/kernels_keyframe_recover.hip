// kernels_keyframe_recover.hip — the device side of recovering a lost camera inside the track (include/hnet.h hnet_sessions_keyframe_track_recover;
// DESIGN 7u).  Four kernels between the unchanged launches of a track (7p, 7q) and of an oriented relocalisation (7r, 7s): the track's decision in its
// deferred form (the lost sessions commit T0 and keep T1 aside), the relocalisation's thumbnails with every candidate of a session that is not lost
// marked absent, the finish that selects between "T0 | RECOVERED" and T1 and assembles the call's one output array, and the map's note for the sessions
// whose T1 was restored.  The per-slot kernels are one wavefront each, fp64 on lane 0, and like kernels_keyframe.hip this file is built with
// -ffp-contract=off: decide_deferred and finish are the host reference's operations in its order.  No atomics, no LDS, nothing waits on another
// workgroup, nothing spins; every id, ring slot and map slot is tested against its table.  The host side that enqueues these kernels is capi_keyframe.hip.
#include "keyframe_recover_dev.h"

namespace hnet {

namespace kf = hnet_keyframe;
namespace km = hnet_keyframe_map;
namespace ps = hnet_search;
namespace kr = hnet_keyframe_recovery;

namespace {
constexpr int REC_DOUBLES = (int)(sizeof(RobustRec) / sizeof(double));
constexpr int TRACK_WORDS = (int)(sizeof(KeyTrack) / 4);
constexpr int THUMB_BLOCKS = (ps::TPIX + 255) / 256;                 // 5 workgroups of 256 threads per thumbnail
static_assert(sizeof(RobustRec) % sizeof(double) == 0 && offsetof(KeyTrack, rec) == 0 && sizeof(KeyTrack) % sizeof(double) == 0, "KeyTrack: the record first, as doubles");
static_assert(sizeof(KeyTrack) % 4 == 0 && sizeof(OrientedRelocRec) == (size_t)kr::RELOC_WORDS * 4 && offsetof(RecoverRec, track) == 0, "records as 32-bit words");
static_assert(ps::STEP == 8 && ps::TW * ps::STEP == IMG_W && ps::TH * ps::STEP == IMG_H, "a thumbnail pixel is an 8 x 8 block of the frame");

__device__ inline bool map_ok(const MapStore& map) { return map.img != nullptr && map.capacity >= km::MIN_CAPACITY && map.capacity <= km::MAX_CAPACITY; }

// thumbnail pixel `pix` of the frame at src (8-byte aligned), as kernels_photo_search.hip makes it: the block's rows as 8-byte loads, then the cascade of
// hnet_align::down4 on the dwords (byte k of row r is (w[2 r + (k >> 2)] >> 8 (k & 3)) & 255)
__device__ __forceinline__ uint8_t thumb_from_frame(const uint8_t* src, int pix) {
    const int v = pix / ps::TW, u = pix - v * ps::TW;
    uint32_t w[16];
    const uint8_t* p = src + (size_t)(ps::STEP * v) * IMG_W + ps::STEP * u;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const uint2 q = *reinterpret_cast<const uint2*>(p + r * IMG_W);
        w[2 * r] = q.x;
        w[2 * r + 1] = q.y;
    }
    uint32_t l2[4];
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int i = 0; i < 2; i++) {
            uint32_t l1[4];
#pragma unroll
            for (int b = 0; b < 2; b++) {
                const uint32_t t = w[2 * (4 * j + 2 * b) + i], d = w[2 * (4 * j + 2 * b + 1) + i];      // four pixels of the upper and of the lower row
                l1[2 * b] = hnet_align::down4(t & 0xFFu, (t >> 8) & 0xFFu, d & 0xFFu, (d >> 8) & 0xFFu);
                l1[2 * b + 1] = hnet_align::down4((t >> 16) & 0xFFu, t >> 24, (d >> 16) & 0xFFu, d >> 24);
            }
            l2[2 * j + i] = hnet_align::down4(l1[0], l1[1], l1[2], l1[3]);
        }
    return hnet_align::down4(l2[0], l2[1], l2[2], l2[3]);
}
}  // namespace

// keyframe_decide_kernel with the deferred decision
__global__ __launch_bounds__(KEY_THREADS) void recover_decide_kernel(KeyTable tab, int n, int n_sessions, const RobustRec* __restrict__ rec, const float* x0, KeyOpts opts,
                                                                     KeyState* state, KeyTrack* out, int32_t* __restrict__ copy, RecoverStash* __restrict__ stash,
                                                                     int32_t* __restrict__ active) {
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
        kr::stash_zero(stash[b]);
        copy[b] = 0;
        active[b] = 0;
        return;
    }
    int act = 0;
    copy[b] = kr::decide_deferred(state[id], x0 + (size_t)b * 8, rec[b], opts, tab.gap[b] != 0, state[id], out[b], stash[b], act);
    active[b] = act;
}

// grid (THUMB_BLOCKS * (M + 2), n): reloc_thumbs_kernel behind active[b]
__global__ __launch_bounds__(256) void recover_thumbs_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ slot, int n_sessions,
                                                             const int32_t* __restrict__ active, const KeyState* __restrict__ state, const uint8_t* __restrict__ key,
                                                             MapStore map, const uint8_t* __restrict__ ring, int n_slots, uint8_t* __restrict__ thumbs,
                                                             int32_t* __restrict__ valid) {
    const int M = map_ok(map) ? map.capacity : 0;
    const int j = blockIdx.x / THUMB_BLOCKS, pix = (blockIdx.x - j * THUMB_BLOCKS) * 256 + threadIdx.x, b = blockIdx.y;
    if (j > M + 1) return;                                                // (the grid is the host's M + 2)
    const int id = ids[b], sc = slot[b];
    const bool call_ok = active[b] != 0 && id >= 0 && id < n_sessions && id < map.n_sessions && sc >= 0 && sc < n_slots;
    const uint8_t* src = nullptr;
    if (call_ok) {
        if (j == 0) {
            if (state[id].has_key != 0) src = key + (size_t)id * NPIX;
        } else if (j <= M) {
            const int ms = j - 1;
            if (map.entry[(size_t)id * M + ms].valid != 0 && ms != map.state[id].cur_slot) src = map.img + ((size_t)id * M + ms) * NPIX;
        } else {
            src = ring + (size_t)sc * NPIX;
        }
    }
    if (j <= M && pix == 0) valid[(size_t)b * (M + 1) + j] = src ? 1 : 0;
    if (!src || pix >= ps::TPIX) return;
    thumbs[((size_t)b * (M + 2) + j) * ps::TPIX + pix] = thumb_from_frame(src, pix);
}

__global__ __launch_bounds__(KEY_THREADS) void recover_finish_kernel(const int32_t* __restrict__ ids, int n, int n_sessions, const int32_t* __restrict__ active,
                                                                     const RecoverStash* __restrict__ stash, const OrientedRelocRec* __restrict__ reloc,
                                                                     KeyState* state, KeyTrack* track, int32_t* __restrict__ copy2, int32_t* __restrict__ redo,
                                                                     RecoverRec* __restrict__ out) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return;
    const int id = ids[b];
    const bool act = id >= 0 && id < n_sessions && active[b] != 0;               // (uniform over the wavefront)
    if (t == 0) {
        int c2 = 0, again = 0;
        if (act) {
            c2 = kr::finish(reloc[b].rv.flags, stash[b], state[id], track[b]);
            again = kr::recovered_by(reloc[b].rv.flags) ? 0 : 1;
        }
        copy2[b] = c2;
        redo[b] = again;
    }
    __syncthreads();                                                             // (lane 0's track[b] is what every lane copies)
    const uint32_t* ts = reinterpret_cast<const uint32_t*>(track + b);
    const uint32_t* rs = reinterpret_cast<const uint32_t*>(reloc + b);
    uint32_t* o = reinterpret_cast<uint32_t*>(out + b);
    for (int i = t; i < TRACK_WORDS; i += KEY_THREADS) o[i] = ts[i];
    for (int i = t; i < kr::RELOC_WORDS; i += KEY_THREADS) o[TRACK_WORDS + i] = act ? rs[i] : kr::zero_reloc_word(i);
}

// keyframe_map_note_kernel behind redo[b]
__global__ __launch_bounds__(KEY_THREADS) void recover_note_kernel(const int32_t* __restrict__ ids, int n, const KeyTrack* __restrict__ track,
                                                                   const int32_t* __restrict__ copy2, const int32_t* __restrict__ redo,
                                                                   const KeyState* __restrict__ state, MapStore map, int32_t* __restrict__ store) {
    const int b = blockIdx.x;
    if (b >= n || threadIdx.x != 0) return;
    const int id = ids[b];
    int slot = -1;
    if (redo[b] != 0 && id >= 0 && id < map.n_sessions && map_ok(map))
        slot = km::note(track[b].flags, copy2[b], state[id], map.state[id], map.entry + (size_t)id * map.capacity, map.capacity);
    store[b] = slot;
}

hipError_t launch_recover_decide(const KeyTable& tab, int n, int n_sessions, const RobustRec* rec, const float* x0, const KeyOpts& opts, KeyState* state,
                                 KeyTrack* out, int32_t* copy, RecoverStash* stash, int32_t* active, hipStream_t s) {
    if (n < 1 || !stash || !active) return hipErrorInvalidValue;
    hipLaunchKernelGGL(recover_decide_kernel, dim3((unsigned)n), dim3(KEY_THREADS), 0, s, tab, n, n_sessions, rec, x0, opts, state, out, copy, stash, active);
    return hipGetLastError();
}

hipError_t launch_recover_thumbs(const int32_t* ids, const int32_t* slot, int n, int n_sessions, const int32_t* active, const KeyState* state, const uint8_t* key,
                                 const MapStore& map, const uint8_t* ring, int n_slots, uint8_t* thumbs, int32_t* valid, hipStream_t s) {
    const int M = map.img ? map.capacity : 0;
    if (n < 1 || n > 65535 || !active || M < 0 || M > km::MAX_CAPACITY || ((((uintptr_t)key) | (uintptr_t)map.img | (uintptr_t)ring) & 7)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(recover_thumbs_kernel, dim3((unsigned)(THUMB_BLOCKS * (M + 2)), (unsigned)n), dim3(256), 0, s, ids, slot, n_sessions, active, state, key, map,
                       ring, n_slots, thumbs, valid);
    return hipGetLastError();
}

hipError_t launch_recover_finish(const int32_t* ids, int n, int n_sessions, const int32_t* active, const RecoverStash* stash, const OrientedRelocRec* reloc,
                                 KeyState* state, KeyTrack* track, int32_t* copy2, int32_t* redo, RecoverRec* out, hipStream_t s) {
    if (n < 1 || !active || !stash || !reloc || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(recover_finish_kernel, dim3((unsigned)n), dim3(KEY_THREADS), 0, s, ids, n, n_sessions, active, stash, reloc, state, track, copy2, redo, out);
    return hipGetLastError();
}

hipError_t launch_recover_note(const int32_t* ids, int n, const KeyTrack* track, const int32_t* copy2, const int32_t* redo, const KeyState* state,
                               const MapStore& map, int32_t* store, hipStream_t s) {
    if (n < 1 || !redo) return hipErrorInvalidValue;
    hipLaunchKernelGGL(recover_note_kernel, dim3((unsigned)n), dim3(KEY_THREADS), 0, s, ids, n, track, copy2, redo, state, map, store);
    return hipGetLastError();
}

}  // namespace hnet
