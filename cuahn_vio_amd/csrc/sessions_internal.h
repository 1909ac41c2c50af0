// sessions_internal.h — what capi_filters.hip reads of the sessions object of capi_sessions.hip: the object itself (a filter steps on its sessions'
// ring, counts, stamps and sequence numbers) and the checks and tables both files build their calls from.  Nothing here is part of the C ABI.
#pragma once
#include "capi_internal.h"

// ---- sessions: many camera streams on one context (include/hnet.h).  Per session: image count, ring orientation, time stamp, mask sequence number and camera, all
// on the host; the frames live in a device ring of 2 slots per session (slot 2 id + k).  Every device step runs on the context's stream.
struct hnet_sessions {
    hnet_ctx* ctx = nullptr;
    hnet_ctx* iter = nullptr;                  // the iterative model's context (hnet_sessions_set_iterative_model) or null: forwards of iteration > 0, on ctx's stream
    int n = 0;
    uint8_t* ring = nullptr;                   // device [n][2][NPIX]
    // t_push: the stamp of the latest push, whatever the count (NaN: none given; hnet_filters_advance's t_frame)
    struct Sess { int count = 0, curr = 0, cam = -1; double t = -1.0; uint64_t seq = 0; double t_push = NAN; };
    std::vector<Sess> st;
    std::vector<uint8_t> mark;                 // id validation scratch (repeats within one call)
    struct Cam { float* map[2]; int rows, cols; };
    std::vector<Cam> cams;
    const float** d_maps = nullptr;            // device [cams][2]: the map pointers session_remap_kernel reads
    // push: two pinned blocks used in turn (the ev_img pattern of hnet_push_image), each {slot table [n] i32, camera table [n] i32 | frames}, and one device slab
    uint8_t* pin[2] = {nullptr, nullptr};
    size_t pin_cap[2] = {0, 0};
    hipEvent_t ev_pin[2] = {nullptr, nullptr};
    int pin_next = 0;
    uint8_t* slab = nullptr;
    size_t slab_cap = 0;
    // infer: ONE pinned block {priors [n][8] f32 | seq table [n] u64 | pair table [n][2] i32} and its device copy, sized for max_batch
    uint8_t* pin_tab = nullptr;
    uint8_t* d_tab = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hnet_timing timing = {};
    struct hnet_keyframes* kf = nullptr;       // the keyframe store (hnet_sessions_enable_keyframes; capi_keyframe.hip) or null: never enabled
};

namespace capi __attribute__((visibility("hidden"))) {

int sessions_check_ids(hnet_sessions* s, int n, const int32_t* ids);          // n distinct ids in range, n within the context's capacity
int sessions_check_pairs(hnet_sessions* s, int n, const int32_t* ids);        // every listed session has a pair: HNET_ERR_NOT_READY otherwise (HomographyNet.cpp:155-158, per session)
// the keyframe layer's part of hnet_destroy_sessions and hnet_sessions_reset (capi_keyframe.hip); both do nothing when keyframes were never enabled
void keyframes_destroy(hnet_sessions* s);
int keyframes_drop(hnet_sessions* s, int id);
// the (prev, curr) ring slots of session `id`'s pair, as launch_session_gather reads them
inline void sessions_pair(const hnet_sessions* s, int id, int32_t* pair) { pair[0] = 2 * id + (s->st[id].curr ^ 1); pair[1] = 2 * id + s->st[id].curr; }

}  // namespace capi
