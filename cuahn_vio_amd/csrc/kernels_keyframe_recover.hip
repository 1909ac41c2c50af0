// kernels_keyframe_recover.hip — the device side of recovering a lost camera inside the track (include/hnet.h hnet_sessions_keyframe_track_recover;
// DESIGN 7u).  Three kernels between the unchanged launches of a track (7p, 7q) and of an oriented relocalisation (7r, 7s), whose thumbnails kernel
// takes active[] and marks every candidate of a session that is not lost absent: the track's decision in its deferred form (the lost sessions commit T0
// and keep T1 aside; for the track inside a filter step, DESIGN 7y, per session the deferred or the plain form), the finish that selects between "T0 | RECOVERED" and T1 and assembles the call's one output array, and the map's note for the
// sessions whose T1 was restored.  The per-slot kernels are one wavefront each, fp64 on lane 0, and like kernels_keyframe.hip this file is built with
// -ffp-contract=off: decide_deferred and finish are the host reference's operations in its order.  No atomics, no LDS, nothing waits on another
// workgroup, nothing spins; every id, ring slot and map slot is tested against its table.  The host side that enqueues these kernels is capi_keyframe.hip.
#include "keyframe_recover_dev.h"
#include "photo_search_kernel_dev.h"

namespace hnet {

namespace kf = hnet_keyframe;
namespace km = hnet_keyframe_map;
namespace kr = hnet_keyframe_recovery;

namespace {
constexpr int REC_DOUBLES = (int)(sizeof(RobustRec) / sizeof(double));
constexpr int TRACK_WORDS = (int)(sizeof(KeyTrack) / 4);
static_assert(sizeof(RobustRec) % sizeof(double) == 0 && offsetof(KeyTrack, rec) == 0 && sizeof(KeyTrack) % sizeof(double) == 0, "KeyTrack: the record first, as doubles");
static_assert(sizeof(KeyTrack) % 4 == 0 && sizeof(OrientedRelocRec) == (size_t)kr::RELOC_WORDS * 4 && offsetof(RecoverRec, track) == 0, "records as 32-bit words");
}  // namespace

// keyframe_decide_kernel with the deferred decision, or per session (recover_on) the plain one; accepted: null, or where the trials the alignment
// accepted over its levels are kept
__global__ __launch_bounds__(KEY_THREADS) void recover_decide_kernel(KeyTable tab, int n, int n_sessions, const RobustRec* __restrict__ rec, int levels, const float* x0,
                                                                     KeyOpts opts, const int32_t* __restrict__ recover_on, KeyState* state, KeyTrack* out,
                                                                     int32_t* __restrict__ copy, RecoverStash* __restrict__ stash, int32_t* __restrict__ active,
                                                                     int32_t* __restrict__ accepted) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return;
    const int id = tab.ids[b];
    const bool valid = id >= 0 && id < n_sessions;                               // (uniform over the workgroup)
    const bool read = valid && state[id].has_key != 0;                           // (read by every lane before lane 0 writes the state: one wavefront, in order)
    const double* src = reinterpret_cast<const double*>(rec + b);
    double* dst = reinterpret_cast<double*>(out + b);
    for (int i = t; i < REC_DOUBLES; i += KEY_THREADS) dst[i] = read ? src[i] : 0.0;
    if (t != 0) return;
    if (accepted) {
        int acc = 0;
        for (int l = 0; l < levels; l++) acc += rec[(size_t)l * n + b].px.accepted;
        accepted[b] = acc;
    }
    if (!valid) {
        for (int i = REC_DOUBLES; i < (int)(sizeof(KeyTrack) / sizeof(double)); i++) dst[i] = 0.0;
        kr::stash_zero(stash[b]);
        copy[b] = 0;
        active[b] = 0;
        return;
    }
    int act = 0;
    if (!recover_on || recover_on[id] != 0) {
        copy[b] = kr::decide_deferred(state[id], x0 + (size_t)b * 8, rec[b], opts, tab.gap[b] != 0, state[id], out[b], stash[b], act);
    } else {
        copy[b] = kf::decide(state[id], x0 + (size_t)b * 8, rec[b], opts, tab.gap[b] != 0, state[id], out[b]);
        kr::stash_zero(stash[b]);
    }
    active[b] = act;
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
    if (redo[b] != 0 && id >= 0 && id < map.n_sessions && reloc_map_ok(map))
        slot = km::note(track[b].flags, copy2[b], state[id], map.state[id], map.entry + (size_t)id * map.capacity, map.capacity);
    store[b] = slot;
}

hipError_t launch_recover_decide(const KeyTable& tab, int n, int n_sessions, const RobustRec* rec, int levels, const float* x0, const KeyOpts& opts,
                                 const int32_t* recover_on, KeyState* state, KeyTrack* out, int32_t* copy, RecoverStash* stash, int32_t* active, int32_t* accepted,
                                 hipStream_t s) {
    if (n < 1 || levels < 1 || levels > hnet_align::MAX_LEVELS || !stash || !active) return hipErrorInvalidValue;
    hipLaunchKernelGGL(recover_decide_kernel, dim3((unsigned)n), dim3(KEY_THREADS), 0, s, tab, n, n_sessions, rec, levels, x0, opts, recover_on, state, out, copy, stash,
                       active, accepted);
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
