// kernels_keyframe_map.hip — the device side of the keyframe map (include/hnet.h hnet_sessions_enable_keyframe_map, hnet_sessions_keyframe_revisit;
// DESIGN 7q).  Two launches behind a track's commit: the bookkeeping of include/hnet_keyframe_map.h's note and the copy of a new keyframe into its slot
// of the map.  Four launches around the unchanged launch_photo_align_robust for a revisit: the choice of a stored keyframe and the start composed through
// the origin chain, the candidate and the current frame gathered into the staging arrays, decide_revisit on the level-0 record, and the candidate's image
// copied over the session's keyframe on an attach.  The per-slot kernels are one wavefront each, fp64 in registers, and like kernels_keyframe.hip built
// with -ffp-contract=off: every function is the host reference's in its order.  The copy kernels move 16-byte vectors, one per lane.  No atomics, no LDS,
// nothing waits on another workgroup.  The host side that enqueues these kernels is capi_keyframe.hip.
#include "keyframe_map_dev.h"

namespace hnet {

namespace kf = hnet_keyframe;
namespace km = hnet_keyframe_map;

namespace {
constexpr int SV = NPIX / 16;                       // 16-byte vectors per frame
static_assert(NPIX % 16 == 0, "frames must stay 16-byte aligned in the map, the store, the ring and the staging arrays");
constexpr int SV_BLOCKS = (SV + 255) / 256;
constexpr int REC_DOUBLES = (int)(sizeof(RobustRec) / sizeof(double));
static_assert(sizeof(RobustRec) % sizeof(double) == 0 && offsetof(MapRevisit, rec) == 0 && sizeof(MapRevisit) % sizeof(double) == 0, "MapRevisit: the record first, as doubles");
static_assert(KEY_THREADS == km::GRID_POINTS, "one lane per grid point, one wavefront per slot");

__device__ inline bool map_ok(const MapStore& map) { return map.capacity >= km::MIN_CAPACITY && map.capacity <= km::MAX_CAPACITY; }
}  // namespace

__global__ __launch_bounds__(KEY_THREADS) void keyframe_map_note_kernel(const int32_t* __restrict__ ids, int n, const KeyTrack* __restrict__ out,
                                                                        const int32_t* __restrict__ copy, const KeyState* __restrict__ state, MapStore map,
                                                                        int32_t* __restrict__ store) {
    const int b = blockIdx.x;
    if (b >= n || threadIdx.x != 0) return;
    const int id = ids[b];
    int slot = -1;
    if (id >= 0 && id < map.n_sessions && map_ok(map))
        slot = km::note(out[b].flags, copy[b], state[id], map.state[id], map.entry + (size_t)id * map.capacity, map.capacity);
    store[b] = slot;
}

__global__ __launch_bounds__(256) void keyframe_map_store_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ store, const uint4* __restrict__ curr,
                                                                 uint4* __restrict__ img, int n_sessions, int capacity) {
    const int v = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    const int slot = store[b];
    if (slot < 0 || slot >= capacity) return;
    const int id = ids[b];
    if (v >= SV || id < 0 || id >= n_sessions) return;
    img[((size_t)id * capacity + slot) * SV + v] = curr[(size_t)b * SV + v];
}

__global__ __launch_bounds__(KEY_THREADS) void keyframe_map_select_kernel(const int32_t* __restrict__ ids, int n, const KeyState* __restrict__ state, MapStore map,
                                                                          int min_grid, float* __restrict__ x0, int32_t* __restrict__ cand, MapRevisit* __restrict__ out) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return;
    const int id = ids[b];
    const bool valid = id >= 0 && id < map.n_sessions && map_ok(map);                    // (uniform over the wavefront, like everything up to the grid test)
    double hb[9];
    for (int k = 0; k < 9; k++) hb[k] = (k & 3) == 0 ? 1.0 : 0.0;
    km::Pick p;
    km::pick_none(p);
    if (valid) {
        const KeyState s = state[id];
        const MapState m = map.state[id];
        const bool have = s.has_key != 0 && km::origin_curr(s, hb);
        for (int slot = 0; slot < map.capacity; slot++) {
            const MapEntry e = map.entry[(size_t)id * map.capacity + slot];
            double G[9];
            float start[8];
            const bool ok = have && km::eligible(m, e, slot) && km::relative(hb, e, G, start);
            const int grid = __popcll(__ballot(ok && km::grid_inside(G, t)));            // (every lane reaches the ballot: ok is uniform)
            if (ok) km::offer(p, slot, e, grid, start, min_grid);
        }
    }
    if (t != 0) return;
    for (int k = 0; k < 8; k++) x0[(size_t)b * 8 + k] = p.start_px[k];
    cand[b] = p.slot;
    out[b].grid = p.grid;
    for (int k = 0; k < 9; k++) out[b].h_origin_before[k] = hb[k];
}

__global__ __launch_bounds__(256) void keyframe_map_gather_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ slot, const int32_t* __restrict__ cand,
                                                                  const uint4* __restrict__ img, int n_sessions, int capacity, const uint4* __restrict__ ring,
                                                                  int n_slots, uint4* __restrict__ prev, uint4* __restrict__ curr) {
    const int v = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    const int c = cand[b];
    if (c < 0 || c >= capacity) return;
    const int id = ids[b], sc = slot[b];
    if (v >= SV || id < 0 || id >= n_sessions || sc < 0 || sc >= n_slots) return;
    const uint4 p = img[((size_t)id * capacity + c) * SV + v], q = ring[(size_t)sc * SV + v];
    prev[(size_t)b * SV + v] = p;
    curr[(size_t)b * SV + v] = q;
}

__global__ __launch_bounds__(KEY_THREADS) void keyframe_map_decide_kernel(const int32_t* __restrict__ ids, int n, const RobustRec* __restrict__ rec, const float* x0,
                                                                          const int32_t* __restrict__ cand, MapOpts opts, KeyState* state, MapStore map, MapRevisit* out,
                                                                          int32_t* __restrict__ attach) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return;
    const int id = ids[b];
    const bool valid = id >= 0 && id < map.n_sessions && map_ok(map);
    int c = cand[b];
    if (!valid || c < 0 || c >= map.capacity) c = -1;
    const double* src = reinterpret_cast<const double*>(rec + b);
    double* dst = reinterpret_cast<double*>(out + b);
    for (int i = t; i < REC_DOUBLES; i += KEY_THREADS) dst[i] = c >= 0 ? src[i] : 0.0;
    if (t != 0) return;
    if (!valid) {
        for (int i = REC_DOUBLES; i < (int)(sizeof(MapRevisit) / sizeof(double)); i++) dst[i] = 0.0;
        out[b].slot = -1;
        out[b].flags = km::RV_NO_CANDIDATE;
        attach[b] = 0;
        return;
    }
    const MapEntry* e = map.entry + (size_t)id * map.capacity;
    attach[b] = km::decide_revisit(state[id], map.state[id], c >= 0 ? e + c : nullptr, c, out[b].grid, x0 + (size_t)b * 8, out[b].h_origin_before, rec[b], opts,
                                   state[id], map.state[id], out[b]);
}

__global__ __launch_bounds__(256) void keyframe_map_attach_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ cand, const int32_t* __restrict__ attach,
                                                                  const uint4* __restrict__ img, int n_sessions, int capacity, uint4* __restrict__ key) {
    const int v = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (attach[b] == 0) return;
    const int id = ids[b], c = cand[b];
    if (v >= SV || id < 0 || id >= n_sessions || c < 0 || c >= capacity) return;
    key[(size_t)id * SV + v] = img[((size_t)id * capacity + c) * SV + v];
}

namespace {
bool bad_grid(int n) { return n < 1 || n > 65535; }
bool unaligned(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return ((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15;
}
}  // namespace

hipError_t launch_keyframe_map_note(const int32_t* ids, int n, const KeyTrack* out, const int32_t* copy, const KeyState* state, const MapStore& map, int32_t* store,
                                    hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyframe_map_note_kernel, dim3((unsigned)n), dim3(KEY_THREADS), 0, s, ids, n, out, copy, state, map, store);
    return hipGetLastError();
}

hipError_t launch_keyframe_map_store(const int32_t* ids, int n, const int32_t* store, const uint8_t* curr, const MapStore& map, hipStream_t s) {
    if (bad_grid(n) || unaligned(curr, map.img)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyframe_map_store_kernel, dim3(SV_BLOCKS, (unsigned)n), dim3(256), 0, s, ids, store, (const uint4*)curr, (uint4*)map.img, map.n_sessions,
                       map.capacity);
    return hipGetLastError();
}

hipError_t launch_keyframe_map_select(const int32_t* ids, int n, const KeyState* state, const MapStore& map, int min_grid, float* x0, int32_t* cand, MapRevisit* out,
                                      hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyframe_map_select_kernel, dim3((unsigned)n), dim3(KEY_THREADS), 0, s, ids, n, state, map, min_grid, x0, cand, out);
    return hipGetLastError();
}

hipError_t launch_keyframe_map_gather(const int32_t* ids, const int32_t* slot, int n, const int32_t* cand, const MapStore& map, const uint8_t* ring, int n_slots,
                                      uint8_t* prev, uint8_t* curr, hipStream_t s) {
    if (bad_grid(n) || unaligned(map.img, ring, prev, curr)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyframe_map_gather_kernel, dim3(SV_BLOCKS, (unsigned)n), dim3(256), 0, s, ids, slot, cand, (const uint4*)map.img, map.n_sessions, map.capacity,
                       (const uint4*)ring, n_slots, (uint4*)prev, (uint4*)curr);
    return hipGetLastError();
}

hipError_t launch_keyframe_map_decide(const int32_t* ids, int n, const RobustRec* rec, const float* x0, const int32_t* cand, const MapOpts& opts, KeyState* state,
                                      const MapStore& map, MapRevisit* out, int32_t* attach, hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyframe_map_decide_kernel, dim3((unsigned)n), dim3(KEY_THREADS), 0, s, ids, n, rec, x0, cand, opts, state, map, out, attach);
    return hipGetLastError();
}

hipError_t launch_keyframe_map_attach(const int32_t* ids, int n, const int32_t* cand, const int32_t* attach, const MapStore& map, uint8_t* key, hipStream_t s) {
    if (bad_grid(n) || unaligned(map.img, key)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyframe_map_attach_kernel, dim3(SV_BLOCKS, (unsigned)n), dim3(256), 0, s, ids, cand, attach, (const uint4*)map.img, map.n_sessions, map.capacity,
                       (uint4*)key);
    return hipGetLastError();
}

}  // namespace hnet
