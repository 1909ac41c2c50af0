// keyframes_internal.h — what the host files of the keyframe layers share of the keyframe store of capi_keyframe.hip: the store itself, its map and its
// scratch, which capi_keyframe_render.hip, capi_keyframe_adjust.hip and capi_keyframe_localise.hip read directly; the base of those three layers, which
// the store owns; the frame of a sessions call (begin_call, finish_call: every call is timed by the store's ONE event pair, each ends in a stream
// synchronisation); the {ids | curr ring slot} table and the layout of the operator-level upload block.  Nothing here is part of the C ABI.
#pragma once
#include "sessions_internal.h"
#include "keyframe_render_dev.h"
#include "keyframe_adjust_dev.h"
#include "keyframe_upload.h"

namespace capi __attribute__((visibility("hidden"))) {

static_assert(KeyUpload::ENTRY_BYTES == sizeof(hnet::MapEntry) && KeyUpload::SEED_BYTES == sizeof(hnet::AdjustRec) && KeyUpload::IMAGE_BYTES == hnet::NPIX &&
              KeyUpload::INFOS_BYTES == (size_t)hnet::ADJUST_MAX_PAIRS * hnet::ADJUST_INFO * sizeof(double), "keyframe_upload.h lays out the device's types");

// a track's table {step [n][8] f32 | ids [n] | curr ring slot [n] | gap [n]}
inline size_t table_bytes(int n) { return (size_t)n * (8 * sizeof(float) + 3 * sizeof(int32_t)); }

// the robust alignment's scratch for max_batch pairs: the store's, lent to every layer that aligns between the store's own calls
struct AlignScratch { hnet::RobustRec* rec; hnet::RobustStart* start; hnet::RobustWork* work; hnet::RobustSums* part; float* x0; };

// the sections of the store's scratch for max_batch B: the alignment's, as capi_filters.hip sizes them for 7o, then the call's table, start, records and copy flags
struct KeyScratch {
    hnet::RobustRec* rec; hnet::RobustStart* start; hnet::RobustWork* work; hnet::RobustSums* part; float* x0; uint8_t* tab; hnet::KeyTrack* out; int32_t* copy;
    size_t bytes;
    KeyScratch(uint8_t* b, int B) {
        Carver cv{b};
        rec = cv.take<hnet::RobustRec>((size_t)HNET_ALIGN_MAX_LEVELS * B);
        start = cv.take<hnet::RobustStart>(B);
        work = cv.take<hnet::RobustWork>(B);
        part = cv.take<hnet::RobustSums>((size_t)B * hnet::PHOTO_SLICES);
        x0 = cv.take<float>((size_t)B * 8);
        tab = cv.take(table_bytes(B));
        out = cv.take<hnet::KeyTrack>(B);
        copy = cv.take<int32_t>(B);
        bytes = cv.used;
    }
    AlignScratch align() const { return AlignScratch{rec, start, work, part, x0}; }
};

// a layer on top of the map (render, adjust, localise): its own file defines its buffers behind this base and allocates them from `mem` at its enable;
// the store holds the pointer and deletes it
struct KeyLayer {
    DevMem mem;
    virtual ~KeyLayer() = default;
};

// a scratch on the device and the pinned blocks of a call's table and of its records [B], with their owner: what the store, its map and the
// relocalisations each hold for their calls
struct KeyBlocks {
    DevMem mem;
    uint8_t* scratch = nullptr;
    uint8_t *pin_in = nullptr, *pin_out = nullptr;
    hipError_t alloc(size_t scratch_bytes, size_t in_bytes, size_t out_bytes) {
        hipError_t e = mem.alloc(&scratch, scratch_bytes);
        if (e == hipSuccess) e = mem.alloc_pinned(&pin_in, in_bytes);
        if (e == hipSuccess) e = mem.alloc_pinned(&pin_out, out_bytes);
        return e;
    }
};

// the map of a store (hnet_sessions_enable_keyframe_map): sized at its enable, for N sessions, M slots each and max_batch B; the sections of
// MapScratch, a revisit's table and its records
struct KeyMap : KeyBlocks {
    hnet::MapStore dev = {nullptr, nullptr, nullptr, 0, 0};    // device: images [N][M][NPIX], entries [N][M], states [N]; all zeroed at enable
};

struct KeyReloc;       // capi_keyframe.hip: the scratch of the relocalisations,
struct KeyFine;        // of the fine relocalise,
struct KeyInstepWork;  // and the working copies of an in-step track with recovery

}  // namespace capi

// the store: everything is sized at enable, for the sessions' count N and the context's max_batch B; the sections of KeyScratch, one call's table and
// its records
struct __attribute__((visibility("hidden"))) hnet_keyframes : capi::KeyBlocks {
    capi::KeyMap* map = nullptr;               // the keyframe map or null: never enabled
    capi::KeyReloc* reloc = nullptr;           // the relocalisation's scratch or null: none of its calls was ever made
    capi::KeyFine* fine = nullptr;             // the fine relocalise's scratch or null: the call was never made
    capi::KeyInstepWork* instep = nullptr;     // the in-step recovery's working copies or null: no filter ever turned it on
    capi::KeyLayer* render = nullptr;          // KeyRender (capi_keyframe_render.hip) or null: hnet_sessions_enable_keyframe_render was never called
    capi::KeyLayer* adjust = nullptr;          // KeyAdjust (capi_keyframe_adjust.hip) or null: hnet_sessions_enable_keyframe_adjust was never called
    capi::KeyLayer* localise = nullptr;        // KeyLocalise (capi_keyframe_localise.hip) or null: hnet_sessions_enable_keyframe_localise was never called
    uint8_t* key = nullptr;                    // device [N][NPIX], zeroed at enable
    hnet::KeyState* state = nullptr;           // device [N], zeroed at enable (has_key = 0)
    hipEvent_t ev[2] = {nullptr, nullptr};     // around the launch sequence of the last call of the store or of a layer: events of its own, every hnet_timing stays as it was
    double ms = 0.0;
    // host mirror of what the device state decides deterministically: whether the session holds a keyframe, and its image count at its previous track
    std::vector<uint8_t> has_key;
    std::vector<int> count_at_track;
    ~hnet_keyframes();                         // capi_keyframe.hip: the map, the scratches and the layers go with the store
};

namespace capi __attribute__((visibility("hidden"))) {

// what a layer's kernels read of a store with a map (the localise's MapStore is k->map->dev itself)
inline hnet::RenderSource render_source(const hnet_keyframes* k) {
    const hnet::MapStore& m = k->map->dev;
    return hnet::RenderSource{m.img, m.entry, k->state, m.n_sessions, m.capacity};
}
inline hnet::AdjustSource adjust_source(const hnet_keyframes* k) {
    const hnet::MapStore& m = k->map->dev;
    return hnet::AdjustSource{m.img, m.entry, k->state, m.state, m.n_sessions, m.capacity};
}

// every listed session has an image; tracked: and holds a keyframe that its last track took from its latest image (HNET_ERR_NOT_READY otherwise)
int check_listed(hnet_sessions* s, int n, const int32_t* ids, const char* who, bool tracked);
// the {ids [n] | curr ring slot [n]} columns of a call's table; on: null, or per session whether it takes part (the id of one that does not is -1)
inline void slot_table(const hnet_sessions* s, int n, const int32_t* ids, const uint8_t* on, int32_t* tab) {
    for (int i = 0; i < n; i++) {
        const int id = ids[i];
        tab[i] = !on || on[id] ? id : -1;
        tab[n + i] = 2 * id + s->st[id].curr;
    }
}
// the frame of a sessions call.  begin_call: ONE upload, then the store's opening event.  finish_call: the closing event, ONE download of the call's
// results, one synchronisation, the device time between the events into k->ms; out: where the results go, or null (the caller reads pin_out).
// Whatever a call synchronises on in between leaves the pair as it is.
int begin_call(hnet_ctx* c, hnet_keyframes* k, void* d_in, const void* pin_in, size_t bytes);
int finish_call(hnet_ctx* c, hnet_keyframes* k, const void* d_out, void* pin_out, void* out, size_t bytes);

}  // namespace capi
