// capi_keyframe.hip — hnet_keyframe_* and hnet_sessions_*keyframe* of include/hnet.h (keyframe_dev.h, csrc/kernels_keyframe.hip): per session a
// frame held longer than one tick, and one call that aligns each listed session's current frame against it from a composed start and applies the rule of
// include/hnet_keyframe.h on the device.  Additive: a sessions object that never enables keyframes has s->kf == nullptr and allocates and launches nothing here.
// On top of it the keyframe MAP (keyframe_map_dev.h, csrc/kernels_keyframe_map.hip): every keyframe a track takes is kept in one of M slots
// per session, and hnet_sessions_keyframe_revisit aligns the current frame against the stored keyframe with the fewest chain links that is still in view
// and re-attaches the session to it (include/hnet_keyframe_map.h).  Additive again: a store whose map was never enabled has kf->map == nullptr and a track
// allocates, launches and returns what it did.
// And the RELOCALISATION (photo_search_dev.h, csrc/kernels_photo_search.hip): hnet_sessions_keyframe_relocalise searches the current frame's
// thumbnail against the held keyframe's and every stored one's, aligns against the best FOUND candidate from the searched start and re-tracks or
// re-attaches the session (include/hnet_keyframe_reloc.h).
// And the ORIENTED relocalisation (photo_search_oriented_dev.h, csrc/kernels_photo_search_oriented.hip): hnet_sessions_keyframe_relocalise_oriented
// is the same call with the search under a table of orientation hypotheses.
// And the RECOVERY inside the track (keyframe_recover_dev.h, csrc/kernels_keyframe_recover.hip): hnet_sessions_keyframe_track_recover is a track
// whose LOST sessions are relocalised (oriented) before their re-key is committed, in one upload, one download and one synchronisation; every launch
// of the track and of the relocalisation is the unchanged one but the decision and a finish.
// The three share ONE launch sequence (enqueue_relocalise) and ONE scratch (RelocScratch), allocated by whichever of them is called first: a
// store that never relocalises has kf->reloc == nullptr.
// And the FINE stage of the oriented relocalisation (photo_search_fine_dev.h, csrc/kernels_photo_search_fine.hip):
// hnet_sessions_keyframe_relocalise_fine runs enqueue_relocalise with the fine search of the picked candidate between the gather and the alignment, on a
// scratch of its own (FineScratch): a store that never makes the call has kf->fine == nullptr, and RelocScratch is what it was.
// And the track INSIDE a filter step (filters_keyframe_dev.h): capi_filters.hip enqueues the track's unchanged launches through the
// keyframes_instep_* functions below, with the store's own scratch, decide on a copy of the state table and the commits deferred to the accepted attempt.
// And the RECOVERY inside that in-step track: the launches of hnet_sessions_keyframe_track_recover on working copies of the state table and
// of the map's entries and states (KeyInstepWork, allocated by hnet_filters_set_keyframe_recover), every image write deferred to the accepted attempt.
// And the RENDER of a map into a view, its joint ADJUSTMENT and the LOCALISE against the rendered map live in
// capi_keyframe_render.hip, capi_keyframe_adjust.hip and capi_keyframe_localise.hip: the store owns each as a KeyLayer and they read the store, its map
// and its alignment scratch directly (keyframes_internal.h, which also holds the frame every sessions call here and there runs in: begin_call, finish_call).
// The four tracks - the two sessions calls and the in-step track with and without recovery - share ONE launch sequence (enqueue_track), as
// the relocalisations do: what each reads and writes is its RelocTargets, the recovering part its KeyRecovery.  The host table of a track has one
// filler (keyframes_table) and the accepted in-step attempt one commit (keyframes_instep_commit).
#include "keyframes_internal.h"
#include "keyframe_recover_dev.h"
#include "photo_search_fine_dev.h"
#include "filters_keyframe_dev.h"

#include <memory>

using namespace hnet;
using namespace capi;

static_assert(sizeof(hnet_keyframe_track) == sizeof(KeyTrack) && offsetof(hnet_keyframe_track, start_px) == offsetof(KeyTrack, start_px) &&
              offsetof(hnet_keyframe_track, key_px) == offsetof(KeyTrack, key_px) && offsetof(hnet_keyframe_track, h_origin_curr) == offsetof(KeyTrack, h_origin_curr) &&
              offsetof(hnet_keyframe_track, overlap) == offsetof(KeyTrack, overlap) && offsetof(hnet_keyframe_track, flags) == offsetof(KeyTrack, flags) &&
              sizeof(hnet_keyframe_opts) == sizeof(KeyOpts) && offsetof(hnet_keyframe_opts, levels) == offsetof(KeyOpts, levels) &&
              offsetof(hnet_keyframe_opts, max_age) == offsetof(KeyOpts, max_age) && offsetof(hnet_keyframe_opts, rekey_overlap) == offsetof(KeyOpts, rekey_overlap) &&
              offsetof(hnet_keyframe_opts, max_mse) == offsetof(KeyOpts, max_mse), "hnet_keyframe_track / _opts are the layouts of include/hnet_keyframe.h");
static_assert((int)HNET_KF_FIRST == hnet_keyframe::FIRST && (int)HNET_KF_REKEYED == hnet_keyframe::REKEYED && (int)HNET_KF_BRIDGED == hnet_keyframe::BRIDGED &&
              (int)HNET_KF_GAP == hnet_keyframe::GAP && (int)HNET_KF_LOW_OVERLAP == hnet_keyframe::LOW_OVERLAP && (int)HNET_KF_MAX_AGE == hnet_keyframe::MAX_AGE &&
              (int)HNET_KF_NO_START == hnet_keyframe::NO_START && (int)HNET_KF_STOPPED == hnet_keyframe::STOPPED && (int)HNET_KF_MSE_ABOVE_MAX == hnet_keyframe::MSE_ABOVE_MAX &&
              (int)HNET_KF_NON_FINITE == hnet_keyframe::NON_FINITE && (int)HNET_KF_ORIGIN_RESTARTED == hnet_keyframe::ORIGIN_RESTARTED &&
              (int)HNET_KF_LOST == hnet_keyframe::LOST, "HNET_KF_* are the header's flags");
static_assert(sizeof(hnet_keyframe_revisit) == sizeof(MapRevisit) && offsetof(hnet_keyframe_revisit, start_px) == offsetof(MapRevisit, start_px) &&
              offsetof(hnet_keyframe_revisit, h_origin_before) == offsetof(MapRevisit, h_origin_before) &&
              offsetof(hnet_keyframe_revisit, closure_px) == offsetof(MapRevisit, closure_px) && offsetof(hnet_keyframe_revisit, overlap) == offsetof(MapRevisit, overlap) &&
              offsetof(hnet_keyframe_revisit, slot) == offsetof(MapRevisit, slot) && offsetof(hnet_keyframe_revisit, flags) == offsetof(MapRevisit, flags) &&
              sizeof(hnet_keyframe_revisit_opts) == sizeof(MapOpts) && offsetof(hnet_keyframe_revisit_opts, min_grid) == offsetof(MapOpts, min_grid) &&
              offsetof(hnet_keyframe_revisit_opts, min_overlap) == offsetof(MapOpts, min_overlap) &&
              offsetof(hnet_keyframe_revisit_opts, max_closure_px) == offsetof(MapOpts, max_closure_px) && sizeof(hnet_keyframe_map_entry) == sizeof(MapEntry) &&
              offsetof(hnet_keyframe_map_entry, h_origin_key) == offsetof(MapEntry, h_origin_key) && sizeof(hnet_keyframe_map_state) == sizeof(MapState),
              "hnet_keyframe_revisit / _opts / _map_entry / _map_state are the layouts of include/hnet_keyframe_map.h");
static_assert((int)HNET_RV_NO_CANDIDATE == hnet_keyframe_map::RV_NO_CANDIDATE && (int)HNET_RV_ATTACHED == hnet_keyframe_map::RV_ATTACHED &&
              (int)HNET_RV_STOPPED == hnet_keyframe_map::RV_STOPPED && (int)HNET_RV_MSE_ABOVE_MAX == hnet_keyframe_map::RV_MSE_ABOVE_MAX &&
              (int)HNET_RV_NON_FINITE == hnet_keyframe_map::RV_NON_FINITE && (int)HNET_RV_LOW_OVERLAP == hnet_keyframe_map::RV_LOW_OVERLAP &&
              (int)HNET_RV_CLOSURE_ABOVE_MAX == hnet_keyframe_map::RV_CLOSURE_ABOVE_MAX && (int)HNET_RV_CHAIN == hnet_keyframe_map::RV_CHAIN &&
              (int)HNET_RV_REJECTED == hnet_keyframe_map::RV_REJECTED, "HNET_RV_* are the header's flags");

static_assert(sizeof(hnet_keyframe_relocalise) == sizeof(RelocRec) && offsetof(hnet_keyframe_relocalise, search) == offsetof(RelocRec, search) &&
              offsetof(hnet_keyframe_relocalise, target) == offsetof(RelocRec, target) && offsetof(hnet_keyframe_relocalise, n_found) == offsetof(RelocRec, n_found) &&
              sizeof(hnet_keyframe_relocalise_opts) == sizeof(RelocOpts) && offsetof(hnet_keyframe_relocalise_opts, levels) == offsetof(RelocOpts, levels) &&
              offsetof(hnet_keyframe_relocalise_opts, search) == offsetof(RelocOpts, search) &&
              offsetof(hnet_keyframe_relocalise_opts, min_overlap) == offsetof(RelocOpts, min_overlap) &&
              offsetof(hnet_keyframe_relocalise_opts, max_closure_px) == offsetof(RelocOpts, max_closure_px),
              "hnet_keyframe_relocalise / _opts are the layouts of include/hnet_keyframe_reloc.h");
static_assert((int)HNET_RL_NO_CANDIDATE == hnet_keyframe_reloc::RL_NO_CANDIDATE && (int)HNET_RL_ATTACHED == hnet_keyframe_reloc::RL_ATTACHED &&
              (int)HNET_RL_STOPPED == hnet_keyframe_reloc::RL_STOPPED && (int)HNET_RL_MSE_ABOVE_MAX == hnet_keyframe_reloc::RL_MSE_ABOVE_MAX &&
              (int)HNET_RL_NON_FINITE == hnet_keyframe_reloc::RL_NON_FINITE && (int)HNET_RL_LOW_OVERLAP == hnet_keyframe_reloc::RL_LOW_OVERLAP &&
              (int)HNET_RL_CLOSURE_ABOVE_MAX == hnet_keyframe_reloc::RL_CLOSURE_ABOVE_MAX && (int)HNET_RL_CHAIN == hnet_keyframe_reloc::RL_CHAIN &&
              (int)HNET_RL_RETRACKED == hnet_keyframe_reloc::RL_RETRACKED && (int)HNET_RL_REJECTED == hnet_keyframe_reloc::RL_REJECTED,
              "HNET_RL_* are the header's flags");
static_assert(sizeof(hnet_keyframe_relocalise_oriented) == sizeof(OrientedRelocRec) && offsetof(hnet_keyframe_relocalise_oriented, search) == offsetof(OrientedRelocRec, search) &&
              offsetof(hnet_keyframe_relocalise_oriented, target) == offsetof(OrientedRelocRec, target) &&
              offsetof(hnet_keyframe_relocalise_oriented, n_found) == offsetof(OrientedRelocRec, n_found),
              "hnet_keyframe_relocalise_oriented is 7r's record around the oriented search record");
static_assert(sizeof(hnet_keyframe_relocalise_fine) == sizeof(FineRelocRec) && offsetof(hnet_keyframe_relocalise_fine, fine) == offsetof(FineRelocRec, fine),
              "hnet_keyframe_relocalise_fine is the oriented relocalise's record followed by the fine part");
static_assert(sizeof(hnet_keyframe_recover) == sizeof(RecoverRec) && offsetof(hnet_keyframe_recover, reloc) == offsetof(RecoverRec, reloc) &&
              sizeof(hnet_keyframe_recover_opts) == sizeof(RecoverOpts) && offsetof(hnet_keyframe_recover_opts, reloc) == offsetof(RecoverOpts, reloc) &&
              (int)HNET_KF_RECOVERED == hnet_keyframe_recovery::RECOVERED, "hnet_keyframe_recover / _opts are the layouts of include/hnet_keyframe_recover.h");

namespace capi __attribute__((visibility("hidden"))) {

// the scratch of the relocalisation (allocated by the first relocalise, oriented relocalise or track with recovery), for max_batch B and the largest
// map: the sections of RelocScratch, the largest call's table and its records
struct KeyReloc : KeyBlocks {};
// the scratch of the fine relocalise (allocated by the first hnet_sessions_keyframe_relocalise_fine), for max_batch B: the sections of FineScratch, the
// call's table and its records
struct KeyFine : KeyBlocks {};

// the working copies of an in-step track with recovery: the map's entries [N][M] and states [N]; null without a map.  Allocated by whichever comes
// second of keyframes_instep_recover_ensure and hnet_sessions_enable_keyframe_map (instep_map_alloc)
struct KeyInstepWork {
    DevMem mem;
    MapEntry* entry = nullptr;
    MapState* state = nullptr;
};

}  // namespace capi

// (hnet_destroy_sessions has set the device and drained the stream)
hnet_keyframes::~hnet_keyframes() {
    delete instep;
    delete render;
    delete adjust;
    delete localise;
    delete map;
    delete reloc;
    delete fine;
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
}

namespace {

// the table of a call of n slots inside a block that holds it
KeyTable table_view(const uint8_t* b, int n) {
    const float* step = reinterpret_cast<const float*>(b);
    const int32_t* ids = reinterpret_cast<const int32_t*>(step + (size_t)8 * n);
    return KeyTable{step, ids, ids + n, ids + 2 * (size_t)n};
}

// the map's own scratch for max_batch B: a revisit's table {ids | curr ring slot}, and per slot the candidate, the store slot of a track's new keyframe,
// the attach flag and the revisit's record.  The alignment's scratch and the start offsets are the store's (KeyScratch).
size_t map_table_bytes(int n) { return (size_t)n * 2 * sizeof(int32_t); }
struct MapScratch {
    int32_t *tab, *cand, *store, *attach; MapRevisit* out; size_t bytes;
    MapScratch(uint8_t* b, int B) {
        Carver cv{b};
        tab = cv.take<int32_t>((size_t)B * 2);
        cand = cv.take<int32_t>(B);
        store = cv.take<int32_t>(B);
        attach = cv.take<int32_t>(B);
        out = cv.take<MapRevisit>(B);
        bytes = cv.used;
    }
};

// the relocalisation's own scratch for max_batch B, one layout for its three calls.  The call's table: {ids | curr ring slot} of a relocalise, with
// {hypotheses [<= 64]} behind it of an oriented one, {step | ids | curr slot | gap | (padding to 8 bytes) | hypotheses} of a track with recovery.  Per slot
// the thumbnails of up to 9 candidates and of the current frame, whether each candidate exists, per candidate the records of up to 64 entries (oriented)
// and its search record, the pick (candidate index and map slot), the attach flag and the relocalisation's record; srec and out hold plain or oriented
// records and are sized for the oriented ones.  Then what only the track with recovery uses: per slot T1's stash, whether the relocalisation runs, the
// second commit's copy flag, whether T1 was restored, the second store's map slot and the call's record.  The alignment's scratch, the start offsets,
// the track records and the first copy flags are the store's (KeyScratch); the first store's map slots are the map's (MapScratch).
size_t recover_ids_bytes(int n) { return (table_bytes(n) + 7) & ~(size_t)7; }
size_t recover_table_bytes(int n, int n_hyp) { return recover_ids_bytes(n) + (size_t)n_hyp * sizeof(SearchHyp); }
struct RelocScratch {
    uint8_t *tab, *thumbs, *srec, *out; int32_t *valid, *cand, *mslot, *attach; SearchRec* hrec;
    RecoverStash* stash; int32_t *active, *copy2, *redo, *store2; RecoverRec* rout; size_t bytes;
    RelocScratch(uint8_t* b, int B) {
        Carver cv{b};
        tab = cv.take(recover_table_bytes(B, SEARCH_MAX_HYP));
        thumbs = cv.take((size_t)B * (RELOC_MAX_CANDIDATES + 1) * THUMB_BYTES);
        valid = cv.take<int32_t>((size_t)B * RELOC_MAX_CANDIDATES);
        hrec = cv.take<SearchRec>((size_t)B * RELOC_MAX_CANDIDATES * SEARCH_MAX_HYP);
        srec = cv.take((size_t)B * RELOC_MAX_CANDIDATES * sizeof(OrientedRec));
        cand = cv.take<int32_t>(B);
        mslot = cv.take<int32_t>(B);
        attach = cv.take<int32_t>(B);
        out = cv.take((size_t)B * sizeof(OrientedRelocRec));
        stash = cv.take<RecoverStash>(B);
        active = cv.take<int32_t>(B);
        copy2 = cv.take<int32_t>(B);
        redo = cv.take<int32_t>(B);
        store2 = cv.take<int32_t>(B);
        rout = cv.take<RecoverRec>(B);
        bytes = cv.used;
    }
};
static_assert(sizeof(OrientedRec) >= sizeof(SearchRec) && sizeof(OrientedRelocRec) >= sizeof(RelocRec) && sizeof(RecoverRec) >= sizeof(OrientedRelocRec),
              "RelocScratch and the pinned blocks are sized by the widest records");

// the fine relocalise's own scratch for max_batch B.  The call's table {ids | curr ring slot | hypotheses [<= 64] | fine table [<= 64][<= 9]}: ONE upload,
// so the oriented table lies here and not in RelocScratch.  Per slot the level-2 thumbnails of the picked candidate [B] and of the current frame [B], the
// records of up to 9 fine entries, and the call's record.  Everything else is RelocScratch's and the store's.
size_t fine_table_bytes(int n, int n_hyp, int n_fine) { return map_table_bytes(n) + (size_t)n_hyp * (1 + n_fine) * sizeof(SearchHyp); }
struct FineScratch {
    uint8_t *tab, *thumbs; FineEntry* ent; FineRelocRec* out; size_t bytes;
    FineScratch(uint8_t* b, int B) {
        Carver cv{b};
        tab = cv.take(fine_table_bytes(B, SEARCH_MAX_HYP, FINE_MAX));
        thumbs = cv.take((size_t)2 * B * FINE_THUMB_BYTES);
        ent = cv.take<FineEntry>((size_t)B * FINE_MAX);
        out = cv.take<FineRelocRec>(B);
        bytes = cv.used;
    }
};
// what enqueue_relocalise runs between the gather and the alignment of a fine relocalise
struct FineStage { const FineScratch* fw; FineOpts fo; const SearchHyp* d_fine; };

// the working copies of the map m for N sessions; on failure w is as it was
hipError_t instep_map_alloc(KeyInstepWork* w, const KeyMap* m, int N) {
    if (w->entry) return hipSuccess;
    DevMem got;
    MapEntry* en = nullptr;
    MapState* st = nullptr;
    hipError_t e = got.alloc(&en, (size_t)N * m->dev.capacity);
    if (e == hipSuccess) e = got.alloc(&st, (size_t)N);
    if (e != hipSuccess) return e;
    w->mem.adopt(got);
    w->entry = en;
    w->state = st;
    return hipSuccess;
}

// o <- *opts with its pads zeroed, or the context's error; name: what the caller calls the struct ("opts", "opts.reloc")
int reloc_check_opts(hnet_ctx* c, const hnet_keyframe_relocalise_opts* opts, const char* who, const char* name, RelocOpts& o) {
    const int rc = photo_robust_check_opts(c, &opts->align, who);
    if (rc != HNET_OK) return rc;
    memcpy(&o, opts, sizeof o);
    if (!hnet_search::opts_valid(o.search))
        return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": " + name +
                                                 ".search: 0 <= radius_x <= 30, 0 <= radius_y <= 20, 16 <= min_overlap <= 1120, -1 <= min_score <= 1, 0 <= min_margin <= 2");
    if (!hnet_keyframe_reloc::opts_valid(o))
        return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": " + name + ": 1 <= levels <= 4, 0 <= min_overlap <= 1, max_mse and max_closure_px >= 0 and finite");
    o.pad = 0;
    o.search.pad = 0;
    return HNET_OK;
}

// a relocalisation's scratch (KeyReloc, KeyFine), allocated by the first call that needs it, before that call enqueues anything
template <class Blocks>
int blocks_ensure(hnet_ctx* c, Blocks*& slot, size_t scratch_bytes, size_t in_bytes, size_t out_bytes, const char* who) {
    if (slot) return HNET_OK;
    auto b = std::make_unique<Blocks>();
    const hipError_t e = b->alloc(scratch_bytes, in_bytes, out_bytes);
    if (e != hipSuccess) return fail(c, HNET_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    slot = b.release();
    return HNET_OK;
}
int reloc_ensure(hnet_ctx* c, hnet_keyframes* k, const char* who) {
    const int B = c->cfg.max_batch;
    return blocks_ensure(c, k->reloc, RelocScratch(nullptr, B).bytes, recover_table_bytes(B, SEARCH_MAX_HYP), (size_t)B * sizeof(RecoverRec), who);
}
int fine_ensure(hnet_ctx* c, hnet_keyframes* k, const char* who) {
    const int B = c->cfg.max_batch;
    return blocks_ensure(c, k->fine, FineScratch(nullptr, B).bytes, fine_table_bytes(B, SEARCH_MAX_HYP, FINE_MAX), (size_t)B * sizeof(FineRelocRec), who);
}

// what a track or a relocalisation reads and writes besides its scratch: the state table its decisions write, the map whose entries and states its notes
// and decisions write (entry null: none, the sequence has no note), the staging pair of its gather and alignment, and the key images that its commits
// and its attach write in sequence, each with its map store (null: every image write is left to a later commit, keyframes_instep_commit)
struct RelocTargets { KeyState* state; MapStore map; uint8_t *prev, *curr, *commit_key; };
// the store's own tables, the context's staging pair, the commits and the attach into the store: what the sessions calls pass
RelocTargets reloc_targets_store(hnet_sessions* s) {
    hnet_ctx* c = s->ctx;
    hnet_keyframes* k = s->kf;
    const MapStore none = {nullptr, nullptr, nullptr, s->n, 0};
    return RelocTargets{k->state, k->map ? k->map->dev : none, (uint8_t*)c->stage_prev, (uint8_t*)c->stage_curr, k->key};
}

// ONE relocalisation of the n listed slots on the stream, between a call's upload and its download: thumbnails, search, pick, gather, robust alignment,
// decision, attach.  d_ids, d_slot: the call's device table; active: null, or per slot whether it takes part (a track with recovery); d_hyps: null for the
// plain search, with SearchRec in rw.srec and RelocRec in rw.out, or the device table of the oriented one, with OrientedRec and OrientedRelocRec there.
// fs: null, or the fine stage of an oriented call: after the gather the picked candidate and the current frame lie in the staging pair; their level-2
// thumbnails, the fine search on the pick's search record and the fine winner, which writes the fine part into fs->fw->out and the final start over w.x0.
// tg: the state table and the map it reads and writes, the staging pair of its gather and alignment, and the key images the attach writes (null: the
// attach is the later commit's, behind rw.mslot and rw.attach).
int enqueue_relocalise(hnet_sessions* s, const RelocTargets& tg, const RelocScratch& rw, const int32_t* d_ids, const int32_t* d_slot, int n, const int32_t* active,
                       const SearchHyp* d_hyps, int n_hyp, const RelocOpts& o, const FineStage* fs = nullptr) {
    hnet_ctx* c = s->ctx;
    hnet_keyframes* k = s->kf;
    const int B = c->cfg.max_batch, N = s->n;
    const KeyScratch w(k->scratch, B);
    const MapStore& map = tg.map;
    const int M = map.capacity;                // 0 without a map
    const size_t pyr = (size_t)B * PYR_BYTES;
    uint8_t *prev = tg.prev, *curr = tg.curr;
    KeyState* state = tg.state;
    hipStream_t st = c->stream;
    HIPCHK(c, launch_reloc_thumbs(d_ids, d_slot, n, N, active, state, k->key, map, s->ring, 2 * N, rw.thumbs, rw.valid, st));
    if (d_hyps) {
        OrientedRec* srec = reinterpret_cast<OrientedRec*>(rw.srec);
        HIPCHK(c, launch_photo_search_oriented(rw.thumbs, M + 2, M + 2, M + 1, M + 1, n, rw.valid, o.search, d_hyps, n_hyp, rw.hrec, nullptr, st));
        HIPCHK(c, launch_photo_search_winner(rw.hrec, d_hyps, n_hyp, n * (M + 1), rw.valid, srec, st));
        HIPCHK(c, launch_reloc_pick(d_ids, n, N, state, M, rw.valid, srec, w.x0, rw.cand, rw.mslot, reinterpret_cast<OrientedRelocRec*>(rw.out), st));
    } else {
        SearchRec* srec = reinterpret_cast<SearchRec*>(rw.srec);
        HIPCHK(c, launch_photo_search(rw.thumbs, M + 2, M + 2, M + 1, M + 1, n, rw.valid, o.search, srec, nullptr, st));
        HIPCHK(c, launch_reloc_pick(d_ids, n, N, state, M, rw.valid, srec, w.x0, rw.cand, rw.mslot, reinterpret_cast<RelocRec*>(rw.out), st));
    }
    HIPCHK(c, launch_reloc_gather(d_ids, d_slot, n, N, rw.cand, k->key, map, s->ring, 2 * N, prev, curr, st));
    if (fs && d_hyps) {
        const FineScratch& fw = *fs->fw;
        const uint8_t* coarse = rw.out + offsetof(OrientedRelocRec, search);
        HIPCHK(c, launch_photo_fine_thumbs(prev, nullptr, n, n, fw.thumbs, st));
        HIPCHK(c, launch_photo_fine_thumbs(curr, nullptr, n, n, fw.thumbs + (size_t)n * FINE_THUMB_BYTES, st));
        HIPCHK(c, launch_photo_search_fine(fw.thumbs, 1, 1, n, n, coarse, (int)sizeof(OrientedRelocRec), rw.cand, o.search, fs->fo, fs->d_fine, n_hyp, fw.ent, nullptr, st));
        HIPCHK(c, launch_photo_search_fine_winner(fw.ent, n, coarse, (int)sizeof(OrientedRelocRec), rw.cand, fs->fo, fs->d_fine, n_hyp, reinterpret_cast<uint8_t*>(fw.out),
                                                  (int)sizeof(FineRelocRec), (int)offsetof(FineRelocRec, fine), false, w.x0, st));
    }
    HIPCHK(c, launch_photo_align_robust(prev, curr, n, w.x0, o.align, o.levels, c->pyr_scratch, c->pyr_scratch + pyr, w.start, w.part, w.work, w.rec, st));
    if (d_hyps)
        HIPCHK(c, launch_reloc_decide(d_ids, n, N, w.rec, w.x0, rw.cand, o, state, map, reinterpret_cast<OrientedRelocRec*>(rw.out), rw.attach, st));
    else
        HIPCHK(c, launch_reloc_decide(d_ids, n, N, w.rec, w.x0, rw.cand, o, state, map, reinterpret_cast<RelocRec*>(rw.out), rw.attach, st));
    if (k->map && tg.commit_key) HIPCHK(c, launch_keyframe_map_attach(d_ids, n, rw.mslot, rw.attach, map, tg.commit_key, st));
    return HNET_OK;
}

// ONE track of the n slots of the device table `tab` on the stream, between a call's upload and its download: start, gather, robust alignment, decide,
// (commit, map note, map store).  rc: null, or the recovering part - the decision deferred for the lost sessions, then the oriented relocalisation of
// those on T0's state (the others ride through on absent candidates and quiet-NaN starts), T0 | RECOVERED or T1 (launch_recover_finish, the call's
// records in RelocScratch::rout) and T1's commit, note and store for the unrecovered sessions (curr still holds every slot's current frame).  The
// track's and the relocalisation's launches act on disjoint sessions after the first commit.  A track without rc touches no RelocScratch.
// tg: as enqueue_relocalise's.  With tg.commit_key null no image is written: the first commit wrote no image a lost session's search reads, so the
// search reads the images it would have read.
int enqueue_track(hnet_sessions* s, const RelocTargets& tg, const KeyTable& tab, int n, const KeyOpts& o, const KeyRecovery* rc) {
    hnet_ctx* c = s->ctx;
    hnet_keyframes* k = s->kf;
    const int B = c->cfg.max_batch, N = s->n;
    const KeyScratch w(k->scratch, B);
    const RelocScratch rw(rc ? k->reloc->scratch : nullptr, B);
    const MapScratch mw(k->map ? k->map->scratch : nullptr, B);
    const bool notes = k->map && tg.map.entry;
    const size_t pyr = (size_t)B * PYR_BYTES;
    hipStream_t st = c->stream;
    HIPCHK(c, launch_keyframe_start(tab, n, N, k->state, w.x0, st));
    HIPCHK(c, launch_keyframe_gather(tab, n, N, k->key, s->ring, 2 * N, tg.prev, tg.curr, st));
    HIPCHK(c, launch_photo_align_robust(tg.prev, tg.curr, n, w.x0, o.align, o.levels, c->pyr_scratch, c->pyr_scratch + pyr, w.start, w.part, w.work, w.rec, st));
    if (rc)
        HIPCHK(c, launch_recover_decide(tab, n, N, w.rec, o.levels, w.x0, o, rc->recover_on, tg.state, w.out, w.copy, rw.stash, rw.active, rc->accepted, st));
    else
        HIPCHK(c, launch_keyframe_decide(tab, n, N, w.rec, w.x0, o, tg.state, w.out, w.copy, st));
    if (tg.commit_key) HIPCHK(c, launch_keyframe_commit(tab, n, N, w.copy, tg.curr, tg.commit_key, st));
    if (notes) {                               // with a map: the bookkeeping of the new keyframes, and their images into their slots
        HIPCHK(c, launch_keyframe_map_note(tab.ids, n, w.out, w.copy, tg.state, tg.map, mw.store, st));
        if (tg.commit_key) HIPCHK(c, launch_keyframe_map_store(tab.ids, n, mw.store, tg.curr, tg.map, st));
    }
    if (!rc) return HNET_OK;
    if (const int r = enqueue_relocalise(s, tg, rw, tab.ids, tab.slot, n, rw.active, rc->d_hyps, rc->n_hyp, rc->o); r != HNET_OK) return r;
    HIPCHK(c, launch_recover_finish(tab.ids, n, N, rw.active, rw.stash, reinterpret_cast<const OrientedRelocRec*>(rw.out), tg.state, w.out, rw.copy2, rw.redo, rw.rout, st));
    if (tg.commit_key) HIPCHK(c, launch_keyframe_commit(tab, n, N, rw.copy2, tg.curr, tg.commit_key, st));
    if (notes) {
        HIPCHK(c, launch_recover_note(tab.ids, n, w.out, rw.copy2, rw.redo, tg.state, tg.map, rw.store2, st));
        if (tg.commit_key) HIPCHK(c, launch_keyframe_map_store(tab.ids, n, rw.store2, tg.curr, tg.map, st));
    }
    return HNET_OK;
}

// hyps null with n_hyp 0: the identity entry alone, made in `identity`
void default_table(const hnet_photo_search_hyp*& hyps, int& n_hyp, SearchHyp& identity) {
    if (hyps || n_hyp != 0) return;
    hnet_search_oriented::make_hyp(0.0, 1.0, identity);
    hyps = reinterpret_cast<const hnet_photo_search_hyp*>(&identity);
    n_hyp = 1;
}

// the host table {step | ids | curr slot | gap} of a sessions call's track in a pinned block (step_px null: zero steps)
void table_fill(const hnet_sessions* s, int n, const int32_t* ids, const float* step_px, uint8_t* pin) {
    float* h_step = reinterpret_cast<float*>(pin);
    for (int i = 0; i < 8 * n; i++) h_step[i] = step_px ? step_px[i] : 0.0f;
    keyframes_table(s, n, ids, nullptr, reinterpret_cast<int32_t*>(h_step + (size_t)8 * n));
}

// ONE upload {ids | curr slot | the oriented call's table}, the launch sequence inside the store's own events, ONE download of the records [n], one
// synchronisation.  oriented: under the table hyps [n_hyp], out [n] hnet_keyframe_relocalise_oriented; else the plain call, out [n] hnet_keyframe_relocalise.
int relocalise(hnet_sessions* s, int n, const int32_t* ids, const hnet_keyframe_relocalise_opts* opts, bool oriented, const hnet_photo_search_hyp* hyps,
               int n_hyp, void* out, const char* who) {
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    hnet_keyframes* k = s->kf;
    if (!k) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": keyframes are not enabled (hnet_sessions_enable_keyframes)");
    if (!out || !opts) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": opts / out");
    RelocOpts o;
    int rc = reloc_check_opts(c, opts, who, "opts", o);
    if (rc != HNET_OK) return rc;
    if (oriented && (rc = photo_search_check_table(c, hyps, n_hyp, who)) != HNET_OK) return rc;
    if ((rc = sessions_check_ids(s, n, ids)) != HNET_OK) return rc;
    if ((rc = check_listed(s, n, ids, who, true)) != HNET_OK) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    if ((rc = reloc_ensure(c, k, who)) != HNET_OK) return rc;
    KeyReloc* r = k->reloc;
    const RelocScratch rw(r->scratch, c->cfg.max_batch);
    slot_table(s, n, ids, nullptr, reinterpret_cast<int32_t*>(r->pin_in));
    const size_t head = map_table_bytes(n), tab = oriented ? (size_t)n_hyp * sizeof(SearchHyp) : 0;
    if (oriented) memcpy(r->pin_in + head, hyps, tab);                 // (8 n bytes in front: the table is aligned)
    const int32_t* d_ids = reinterpret_cast<const int32_t*>(rw.tab);
    const SearchHyp* d_hyps = oriented ? reinterpret_cast<const SearchHyp*>(rw.tab + head) : nullptr;
    if ((rc = begin_call(c, k, rw.tab, r->pin_in, head + tab)) != HNET_OK) return rc;
    if ((rc = enqueue_relocalise(s, reloc_targets_store(s), rw, d_ids, d_ids + n, n, nullptr, d_hyps, n_hyp, o)) != HNET_OK) return rc;
    return finish_call(c, k, rw.out, r->pin_out, out, (size_t)n * (oriented ? sizeof(OrientedRelocRec) : sizeof(RelocRec)));
}

// hnet_sessions_keyframe_relocalise_oriented with the fine stage on the picked candidate: ONE upload {ids | curr slot | table | fine table} into the fine
// scratch, the launch sequence inside the store's own events, the oriented records packed in front of the fine parts, ONE download, one synchronisation
int relocalise_fine(hnet_sessions* s, int n, const int32_t* ids, const hnet_keyframe_relocalise_opts* opts, const hnet_photo_search_hyp* hyps, int n_hyp,
                    const hnet_photo_search_fine_opts* fine_opts, const hnet_photo_search_hyp* fine, hnet_keyframe_relocalise_fine* out, const char* who) {
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    hnet_keyframes* k = s->kf;
    if (!k) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": keyframes are not enabled (hnet_sessions_enable_keyframes)");
    if (!out || !opts) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": opts / out");
    RelocOpts o;
    FineStage fs;
    int rc = reloc_check_opts(c, opts, who, "opts", o);
    if (rc != HNET_OK) return rc;
    if ((rc = photo_search_check_table(c, hyps, n_hyp, who)) != HNET_OK) return rc;
    if ((rc = photo_search_fine_check(c, fine_opts, fine, n_hyp, who, fs.fo)) != HNET_OK) return rc;
    if ((rc = sessions_check_ids(s, n, ids)) != HNET_OK) return rc;
    if ((rc = check_listed(s, n, ids, who, true)) != HNET_OK) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    if ((rc = reloc_ensure(c, k, who)) != HNET_OK) return rc;
    if ((rc = fine_ensure(c, k, who)) != HNET_OK) return rc;
    KeyFine* f = k->fine;
    const RelocScratch rw(k->reloc->scratch, c->cfg.max_batch);
    const FineScratch fw(f->scratch, c->cfg.max_batch);
    slot_table(s, n, ids, nullptr, reinterpret_cast<int32_t*>(f->pin_in));
    const size_t head = map_table_bytes(n), tab = (size_t)n_hyp * sizeof(SearchHyp), ftab = tab * fs.fo.n_fine;      // (8 n bytes in front: the tables are aligned)
    memcpy(f->pin_in + head, hyps, tab);
    memcpy(f->pin_in + head + tab, fine, ftab);
    const int32_t* d_ids = reinterpret_cast<const int32_t*>(fw.tab);
    const SearchHyp* d_hyps = reinterpret_cast<const SearchHyp*>(fw.tab + head);
    fs.fw = &fw;
    fs.d_fine = reinterpret_cast<const SearchHyp*>(fw.tab + head + tab);
    if ((rc = begin_call(c, k, fw.tab, f->pin_in, head + tab + ftab)) != HNET_OK) return rc;
    if ((rc = enqueue_relocalise(s, reloc_targets_store(s), rw, d_ids, d_ids + n, n, nullptr, d_hyps, n_hyp, o, &fs)) != HNET_OK) return rc;
    HIPCHK(c, launch_reloc_fine_pack(reinterpret_cast<const OrientedRelocRec*>(rw.out), n, fw.out, c->stream));
    return finish_call(c, k, fw.out, f->pin_out, out, (size_t)n * sizeof(FineRelocRec));
}

}  // namespace

namespace capi {

// (hnet_destroy_sessions has set the device and drained the stream)
void keyframes_destroy(hnet_sessions* s) {
    delete s->kf;
    s->kf = nullptr;
}

int check_listed(hnet_sessions* s, int n, const int32_t* ids, const char* who, bool tracked) {
    hnet_ctx* c = s->ctx;
    const hnet_keyframes* k = s->kf;
    for (int i = 0; i < n; i++) {
        const int id = ids[i];
        if (s->st[id].count < 1) return fail(c, HNET_ERR_NOT_READY, std::string(who) + ": a listed session has no image");
        if (!tracked) continue;
        if (!k->has_key[id]) return fail(c, HNET_ERR_NOT_READY, std::string(who) + ": a listed session holds no keyframe");
        if (s->st[id].count != k->count_at_track[id])
            return fail(c, HNET_ERR_NOT_READY, std::string(who) + ": a listed session's latest image is not the one its last track saw (track it first)");
    }
    return HNET_OK;
}

int begin_call(hnet_ctx* c, hnet_keyframes* k, void* d_in, const void* pin_in, size_t bytes) {
    HIPCHK(c, hipMemcpyAsync(d_in, pin_in, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(k->ev[0], c->stream));
    return HNET_OK;
}

int finish_call(hnet_ctx* c, hnet_keyframes* k, const void* d_out, void* pin_out, void* out, size_t bytes) {
    hipStream_t st = c->stream;
    HIPCHK(c, hipEventRecord(k->ev[1], st));
    HIPCHK(c, hipMemcpyAsync(pin_out, d_out, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, k->ev[0], k->ev[1]));
    k->ms = ms;
    if (out) memcpy(out, pin_out, bytes);
    return HNET_OK;
}

// the session's keyframe and origin chain are dropped: its next track is FIRST.  Stream ordered behind every enqueued track; nothing is synchronised.
int keyframes_drop(hnet_sessions* s, int id) {
    hnet_keyframes* k = s->kf;
    if (!k) return HNET_OK;
    hnet_ctx* c = s->ctx;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipMemsetAsync(k->state + id, 0, sizeof(KeyState), c->stream));
    if (const KeyMap* m = k->map) {            // the session's map goes with its origin: no entry stays valid (the images need no clearing)
        HIPCHK(c, hipMemsetAsync(m->dev.entry + (size_t)id * m->dev.capacity, 0, (size_t)m->dev.capacity * sizeof(MapEntry), c->stream));
        HIPCHK(c, hipMemsetAsync(m->dev.state + id, 0, sizeof(MapState), c->stream));
    }
    k->has_key[id] = 0;
    k->count_at_track[id] = -1;
    return HNET_OK;
}

bool keyframes_enabled(const hnet_sessions* s) { return s->kf != nullptr; }

void keyframes_table(const hnet_sessions* s, int n, const int32_t* ids, const uint8_t* on, int32_t* tab) {
    const hnet_keyframes* k = s->kf;
    slot_table(s, n, ids, on, tab);
    for (int i = 0; i < n; i++) tab[2 * n + i] = k->has_key[ids[i]] && s->st[ids[i]].count != k->count_at_track[ids[i]] + 1 ? 1 : 0;
}

// (the store's events and ms stay the last sessions call's.  A plain track has no working copy of the map: its note waits for the commit; one with
// recovery notes on the working copies, which the relocalisation reads, and every attempt starts from the committed tables)
int keyframes_instep_track(hnet_sessions* s, const KeyTable& tab, int n, const KeyOpts& o, const KeyRecovery* rc, uint8_t* prev, uint8_t* curr, KeyState* state_work,
                           KeyInstep* v) {
    hnet_ctx* c = s->ctx;
    hnet_keyframes* k = s->kf;
    const int B = c->cfg.max_batch, N = s->n;
    hipStream_t st = c->stream;
    MapStore map = {nullptr, nullptr, nullptr, N, 0};
    HIPCHK(c, hipMemcpyAsync(state_work, k->state, (size_t)N * sizeof(KeyState), hipMemcpyDeviceToDevice, st));
    if (const KeyMap* m = rc ? k->map : nullptr) {     // the store's images (read only before the accepted attempt) around the working entries and states
        map = MapStore{m->dev.img, k->instep->entry, k->instep->state, m->dev.n_sessions, m->dev.capacity};
        HIPCHK(c, hipMemcpyAsync(map.entry, m->dev.entry, (size_t)N * map.capacity * sizeof(MapEntry), hipMemcpyDeviceToDevice, st));
        HIPCHK(c, hipMemcpyAsync(map.state, m->dev.state, (size_t)N * sizeof(MapState), hipMemcpyDeviceToDevice, st));
    }
    if (const int r = enqueue_track(s, RelocTargets{state_work, map, prev, curr, nullptr}, tab, n, o, rc); r != HNET_OK) return r;
    const KeyScratch w(k->scratch, B);
    if (rc) *v = KeyInstep{w.rec, rc->o.levels, nullptr, RelocScratch(k->reloc->scratch, B).rout, k->state};
    else *v = KeyInstep{w.rec, o.levels, w.out, nullptr, k->state};
    return HNET_OK;
}

int keyframes_instep_commit(hnet_sessions* s, const KeyTable& tab, int n, bool recovering, const uint8_t* curr, const KeyState* state_work) {
    hnet_ctx* c = s->ctx;
    hnet_keyframes* k = s->kf;
    const int B = c->cfg.max_batch, N = s->n;
    const KeyScratch w(k->scratch, B);
    const RelocScratch rw(recovering ? k->reloc->scratch : nullptr, B);
    const KeyMap* m = k->map;
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(k->state, state_work, (size_t)N * sizeof(KeyState), hipMemcpyDeviceToDevice, st));
    HIPCHK(c, launch_keyframe_commit(tab, n, N, w.copy, curr, k->key, st));
    if (m) {
        const MapScratch mw(m->scratch, B);
        if (recovering) {
            HIPCHK(c, hipMemcpyAsync(m->dev.entry, k->instep->entry, (size_t)N * m->dev.capacity * sizeof(MapEntry), hipMemcpyDeviceToDevice, st));
            HIPCHK(c, hipMemcpyAsync(m->dev.state, k->instep->state, (size_t)N * sizeof(MapState), hipMemcpyDeviceToDevice, st));
        } else {
            HIPCHK(c, launch_keyframe_map_note(tab.ids, n, w.out, w.copy, k->state, m->dev, mw.store, st));
        }
        HIPCHK(c, launch_keyframe_map_store(tab.ids, n, mw.store, curr, m->dev, st));
    }
    if (!recovering) return HNET_OK;
    if (m) HIPCHK(c, launch_keyframe_map_attach(tab.ids, n, rw.mslot, rw.attach, m->dev, k->key, st));
    HIPCHK(c, launch_keyframe_commit(tab, n, N, rw.copy2, curr, k->key, st));
    if (m) HIPCHK(c, launch_keyframe_map_store(tab.ids, n, rw.store2, curr, m->dev, st));
    return HNET_OK;
}

void keyframes_instep_accepted(hnet_sessions* s, int n, const int32_t* ids, const uint8_t* on) {
    hnet_keyframes* k = s->kf;
    for (int i = 0; i < n; i++)
        if (on[ids[i]]) {
            k->has_key[ids[i]] = 1;
            k->count_at_track[ids[i]] = s->st[ids[i]].count;
        }
}

int keyframes_recover_check(hnet_sessions* s, const hnet_keyframe_relocalise_opts* opts, const hnet_photo_search_hyp* hyps, int n_hyp, const char* who, RelocOpts& o,
                            SearchHyp* table, int* n_table) {
    hnet_ctx* c = s->ctx;
    int rc = reloc_check_opts(c, opts, who, "reloc", o);
    if (rc != HNET_OK) return rc;
    SearchHyp identity;
    default_table(hyps, n_hyp, identity);
    if ((rc = photo_search_check_table(c, hyps, n_hyp, who)) != HNET_OK) return rc;
    static_assert(sizeof(hnet_photo_search_hyp) == sizeof(SearchHyp), "the table is copied as it is");
    memset(table, 0, (size_t)SEARCH_MAX_HYP * sizeof(SearchHyp));
    memcpy(table, hyps, (size_t)n_hyp * sizeof(SearchHyp));
    *n_table = n_hyp;
    return HNET_OK;
}

int keyframes_instep_recover_ensure(hnet_sessions* s, const char* who) {
    hnet_ctx* c = s->ctx;
    hnet_keyframes* k = s->kf;
    if (!k) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": keyframes are not enabled (hnet_sessions_enable_keyframes)");
    if (k->instep) return HNET_OK;                 // (a map enabled since then brought its working copies with it: hnet_sessions_enable_keyframe_map)
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    if (const int rc = reloc_ensure(c, k, who); rc != HNET_OK) return rc;
    auto w = std::make_unique<KeyInstepWork>();
    if (const KeyMap* m = k->map) {
        const hipError_t e = instep_map_alloc(w.get(), m, s->n);
        if (e != hipSuccess) return fail(c, HNET_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    }
    k->instep = w.release();
    return HNET_OK;
}

}  // namespace capi

extern "C" {

void hnet_keyframe_default_opts(hnet_keyframe_opts* o) {
    if (!o) return;
    KeyOpts d;
    hnet_keyframe::default_opts(d);
    memcpy(o, &d, sizeof d);
}

int hnet_sessions_enable_keyframes(hnet_sessions* s) {
    const char* who = "hnet_sessions_enable_keyframes";
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    if (s->kf) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": keyframes are already enabled");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const int B = c->cfg.max_batch, N = s->n;
    if (const int rc = ensure_pyr_scratch(c); rc != HNET_OK) return rc;
    auto k = std::make_unique<hnet_keyframes>();
    hipError_t e = k->mem.alloc(&k->key, (size_t)N * NPIX);
    if (e == hipSuccess) e = k->mem.alloc(&k->state, (size_t)N);
    if (e == hipSuccess) e = k->alloc(KeyScratch(nullptr, B).bytes, table_bytes(B), (size_t)B * sizeof(KeyTrack));
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipEventCreate(&k->ev[i]);      // (the one pair of the store and of every layer on it)
    if (e == hipSuccess) e = hipMemsetAsync(k->key, 0, (size_t)N * NPIX, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(k->state, 0, (size_t)N * sizeof(KeyState), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, HNET_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    k->has_key.assign(N, 0);
    k->count_at_track.assign(N, -1);
    s->kf = k.release();
    return HNET_OK;
}

// ONE upload {step | ids | curr slot | gap}, the launch sequence inside the store's own events, ONE download of the records [n], one synchronisation
int hnet_sessions_keyframe_track(hnet_sessions* s, int n, const int32_t* ids, const float* step_px, const hnet_keyframe_opts* opts, hnet_keyframe_track* out) {
    const char* who = "hnet_sessions_keyframe_track";
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    hnet_keyframes* k = s->kf;
    if (!k) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": keyframes are not enabled (hnet_sessions_enable_keyframes)");
    if (!out || !opts) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": opts / out");
    int rc = photo_robust_check_opts(c, &opts->align, who);
    if (rc != HNET_OK) return rc;
    KeyOpts o;
    memcpy(&o, opts, sizeof o);
    if (!hnet_keyframe::opts_valid(o))
        return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": opts: 1 <= levels <= 4, auto_rekey 0 / 1, max_age >= 0, 0 <= rekey_overlap <= 1, max_mse >= 0 and finite");
    if ((rc = sessions_check_ids(s, n, ids)) != HNET_OK) return rc;
    if ((rc = check_listed(s, n, ids, who, false)) != HNET_OK) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const KeyScratch w(k->scratch, c->cfg.max_batch);
    table_fill(s, n, ids, step_px, k->pin_in);
    if ((rc = begin_call(c, k, w.tab, k->pin_in, table_bytes(n))) != HNET_OK) return rc;
    if ((rc = enqueue_track(s, reloc_targets_store(s), table_view(w.tab, n), n, o, nullptr)) != HNET_OK) return rc;
    if ((rc = finish_call(c, k, w.out, k->pin_out, out, (size_t)n * sizeof(KeyTrack))) != HNET_OK) return rc;
    for (int i = 0; i < n; i++) {
        k->has_key[ids[i]] = 1;
        k->count_at_track[ids[i]] = s->st[ids[i]].count;
    }
    return HNET_OK;
}

int hnet_sessions_keyframe_reset(hnet_sessions* s, int id) {
    if (!s) return HNET_ERR_INVALID_ARG;
    if (!s->kf) return fail(s->ctx, HNET_ERR_INVALID_ARG, "hnet_sessions_keyframe_reset: keyframes are not enabled (hnet_sessions_enable_keyframes)");
    if (id < 0 || id >= s->n) return fail(s->ctx, HNET_ERR_INVALID_ARG, "sessions: id out of range");
    return keyframes_drop(s, id);
}

int hnet_sessions_get_keyframe(hnet_sessions* s, int id, uint8_t* out) {
    const char* who = "hnet_sessions_get_keyframe";
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    if (!s->kf) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": keyframes are not enabled (hnet_sessions_enable_keyframes)");
    if (!out || id < 0 || id >= s->n) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": id / out");
    if (!s->kf->has_key[id]) return fail(c, HNET_ERR_NOT_READY, std::string(who) + ": the session holds no keyframe");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipMemcpyAsync(out, s->kf->key + (size_t)id * NPIX, NPIX, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HNET_OK;
}

void hnet_keyframe_revisit_default_opts(hnet_keyframe_revisit_opts* o) {
    if (!o) return;
    MapOpts d;
    hnet_keyframe_map::default_opts(d);
    memcpy(o, &d, sizeof d);
}

int hnet_sessions_enable_keyframe_map(hnet_sessions* s, int capacity) {
    const char* who = "hnet_sessions_enable_keyframe_map";
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    hnet_keyframes* k = s->kf;
    if (!k) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": keyframes are not enabled (hnet_sessions_enable_keyframes)");
    if (k->map) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": the keyframe map is already enabled");
    if (capacity < hnet_keyframe_map::MIN_CAPACITY || capacity > hnet_keyframe_map::MAX_CAPACITY)
        return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": 2 <= capacity <= 8");
    for (int id = 0; id < s->n; id++)
        if (k->has_key[id]) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": a session already holds a keyframe, which would not be in the map");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const int B = c->cfg.max_batch, N = s->n, M = capacity;
    auto m = std::make_unique<KeyMap>();
    m->dev.n_sessions = N;
    m->dev.capacity = M;
    const size_t img = (size_t)N * M * NPIX, ent = (size_t)N * M * sizeof(MapEntry), sta = (size_t)N * sizeof(MapState);
    hipError_t e = m->mem.alloc(&m->dev.img, img);
    if (e == hipSuccess) e = m->mem.alloc(&m->dev.entry, (size_t)N * M);
    if (e == hipSuccess) e = m->mem.alloc(&m->dev.state, (size_t)N);
    if (e == hipSuccess) e = m->alloc(MapScratch(nullptr, B).bytes, map_table_bytes(B), (size_t)B * sizeof(MapRevisit));
    if (e == hipSuccess && k->instep) e = instep_map_alloc(k->instep, m.get(), N);      // (a filter turned the in-step recovery on before the map existed)
    if (e == hipSuccess) e = hipMemsetAsync(m->dev.img, 0, img, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(m->dev.entry, 0, ent, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(m->dev.state, 0, sta, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, HNET_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    k->map = m.release();
    return HNET_OK;
}

// ONE upload {ids | curr slot}, the launch sequence inside the store's events, ONE download of the records [n], one synchronisation
int hnet_sessions_keyframe_revisit(hnet_sessions* s, int n, const int32_t* ids, const hnet_keyframe_revisit_opts* opts, hnet_keyframe_revisit* out) {
    const char* who = "hnet_sessions_keyframe_revisit";
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    hnet_keyframes* k = s->kf;
    if (!k) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": keyframes are not enabled (hnet_sessions_enable_keyframes)");
    KeyMap* m = k->map;
    if (!m) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": the keyframe map is not enabled (hnet_sessions_enable_keyframe_map)");
    if (!out || !opts) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": opts / out");
    int rc = photo_robust_check_opts(c, &opts->align, who);
    if (rc != HNET_OK) return rc;
    MapOpts o;
    memcpy(&o, opts, sizeof o);
    if (!hnet_keyframe_map::opts_valid(o))
        return fail(c, HNET_ERR_INVALID_ARG,
                    std::string(who) + ": opts: 1 <= levels <= 4, 1 <= min_grid <= 64, 0 <= min_overlap <= 1, max_mse and max_closure_px >= 0 and finite");
    if ((rc = sessions_check_ids(s, n, ids)) != HNET_OK) return rc;
    if ((rc = check_listed(s, n, ids, who, true)) != HNET_OK) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const int B = c->cfg.max_batch, N = s->n;
    const KeyScratch w(k->scratch, B);
    const MapScratch mw(m->scratch, B);
    slot_table(s, n, ids, nullptr, reinterpret_cast<int32_t*>(m->pin_in));
    const int32_t *d_ids = mw.tab, *d_slot = mw.tab + n;
    const size_t pyr = (size_t)B * PYR_BYTES;
    uint8_t *prev = (uint8_t*)c->stage_prev, *curr = (uint8_t*)c->stage_curr;
    hipStream_t st = c->stream;
    if ((rc = begin_call(c, k, mw.tab, m->pin_in, map_table_bytes(n))) != HNET_OK) return rc;
    HIPCHK(c, launch_keyframe_map_select(d_ids, n, k->state, m->dev, o.min_grid, w.x0, mw.cand, mw.out, st));
    HIPCHK(c, launch_keyframe_map_gather(d_ids, d_slot, n, mw.cand, m->dev, s->ring, 2 * N, prev, curr, st));
    HIPCHK(c, launch_photo_align_robust(prev, curr, n, w.x0, o.align, o.levels, c->pyr_scratch, c->pyr_scratch + pyr, w.start, w.part, w.work, w.rec, st));
    HIPCHK(c, launch_keyframe_map_decide(d_ids, n, w.rec, w.x0, mw.cand, o, k->state, m->dev, mw.out, mw.attach, st));
    HIPCHK(c, launch_keyframe_map_attach(d_ids, n, mw.cand, mw.attach, m->dev, k->key, st));
    return finish_call(c, k, mw.out, m->pin_out, out, (size_t)n * sizeof(MapRevisit));
}

int hnet_sessions_keyframe_map_info(hnet_sessions* s, int id, hnet_keyframe_map_entry* entries, hnet_keyframe_map_state* map_state) {
    const char* who = "hnet_sessions_keyframe_map_info";
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    if (!s->kf || !s->kf->map) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": the keyframe map is not enabled (hnet_sessions_enable_keyframe_map)");
    if (!entries || !map_state || id < 0 || id >= s->n) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": id / entries / map_state");
    const KeyMap* m = s->kf->map;
    const int M = m->dev.capacity;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipMemcpyAsync(entries, m->dev.entry + (size_t)id * M, (size_t)M * sizeof(MapEntry), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(map_state, m->dev.state + id, sizeof(MapState), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HNET_OK;
}

int hnet_sessions_get_map_keyframe(hnet_sessions* s, int id, int slot, uint8_t* out) {
    const char* who = "hnet_sessions_get_map_keyframe";
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    if (!s->kf || !s->kf->map) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": the keyframe map is not enabled (hnet_sessions_enable_keyframe_map)");
    const KeyMap* m = s->kf->map;
    if (!out || id < 0 || id >= s->n || slot < 0 || slot >= m->dev.capacity) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": id / slot / out");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipMemcpyAsync(out, m->dev.img + ((size_t)id * m->dev.capacity + slot) * NPIX, NPIX, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HNET_OK;
}

void hnet_keyframe_relocalise_default_opts(hnet_keyframe_relocalise_opts* o) {
    if (!o) return;
    RelocOpts d;
    hnet_keyframe_reloc::default_opts(d);
    memcpy(o, &d, sizeof d);
}

int hnet_sessions_keyframe_relocalise(hnet_sessions* s, int n, const int32_t* ids, const hnet_keyframe_relocalise_opts* opts, hnet_keyframe_relocalise* out) {
    return relocalise(s, n, ids, opts, false, nullptr, 0, out, "hnet_sessions_keyframe_relocalise");
}

// hnet_sessions_keyframe_relocalise with the oriented search
int hnet_sessions_keyframe_relocalise_oriented(hnet_sessions* s, int n, const int32_t* ids, const hnet_keyframe_relocalise_opts* opts,
                                               const hnet_photo_search_hyp* hyps, int n_hyp, hnet_keyframe_relocalise_oriented* out) {
    return relocalise(s, n, ids, opts, true, hyps, n_hyp, out, "hnet_sessions_keyframe_relocalise_oriented");
}

// hnet_sessions_keyframe_relocalise_oriented with the fine stage on the picked candidate
int hnet_sessions_keyframe_relocalise_fine(hnet_sessions* s, int n, const int32_t* ids, const hnet_keyframe_relocalise_opts* opts, const hnet_photo_search_hyp* hyps,
                                           int n_hyp, const hnet_photo_search_fine_opts* fine_opts, const hnet_photo_search_hyp* fine,
                                           hnet_keyframe_relocalise_fine* out) {
    return relocalise_fine(s, n, ids, opts, hyps, n_hyp, fine_opts, fine, out, "hnet_sessions_keyframe_relocalise_fine");
}

void hnet_keyframe_recover_default_opts(hnet_keyframe_recover_opts* o) {
    if (!o) return;
    RecoverOpts d;
    hnet_keyframe_recovery::default_opts(d);
    memcpy(o, &d, sizeof d);
}

// hnet_sessions_keyframe_track with the oriented relocalisation of the LOST sessions inside it: ONE upload {step | ids | curr slot | gap | table}, the
// launch sequence inside the store's own events, ONE download of the records [n], one synchronisation.  The track's and the relocalisation's launches act
// on disjoint sessions after the first commit: the sessions that are not lost are committed by it and every candidate of theirs is absent from the
// search; the lost ones hold T0 (no copy) until the finish.
int hnet_sessions_keyframe_track_recover(hnet_sessions* s, int n, const int32_t* ids, const float* step_px, const hnet_keyframe_recover_opts* opts,
                                         const hnet_photo_search_hyp* hyps, int n_hyp, hnet_keyframe_recover* out) {
    const char* who = "hnet_sessions_keyframe_track_recover";
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    hnet_keyframes* k = s->kf;
    if (!k) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": keyframes are not enabled (hnet_sessions_enable_keyframes)");
    if (!out || !opts) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": opts / out");
    int rc = photo_robust_check_opts(c, &opts->track.align, who);
    if (rc != HNET_OK) return rc;
    RecoverOpts o;
    memcpy(&o.track, &opts->track, sizeof o.track);
    if (!hnet_keyframe::opts_valid(o.track))
        return fail(c, HNET_ERR_INVALID_ARG,
                    std::string(who) + ": opts.track: 1 <= levels <= 4, auto_rekey 0 / 1, max_age >= 0, 0 <= rekey_overlap <= 1, max_mse >= 0 and finite");
    if ((rc = reloc_check_opts(c, &opts->reloc, who, "opts.reloc", o.reloc)) != HNET_OK) return rc;
    SearchHyp identity;
    default_table(hyps, n_hyp, identity);
    if ((rc = photo_search_check_table(c, hyps, n_hyp, who)) != HNET_OK) return rc;
    if ((rc = sessions_check_ids(s, n, ids)) != HNET_OK) return rc;
    if ((rc = check_listed(s, n, ids, who, false)) != HNET_OK) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    if ((rc = reloc_ensure(c, k, who)) != HNET_OK) return rc;
    KeyReloc* r = k->reloc;
    const RelocScratch rw(r->scratch, c->cfg.max_batch);
    table_fill(s, n, ids, step_px, r->pin_in);
    const size_t head = recover_ids_bytes(n), tabb = (size_t)n_hyp * sizeof(SearchHyp);
    memset(r->pin_in + table_bytes(n), 0, head - table_bytes(n));
    memcpy(r->pin_in + head, hyps, tabb);
    const KeyRecovery rec{o.reloc, reinterpret_cast<const SearchHyp*>(rw.tab + head), n_hyp, nullptr, nullptr};
    if ((rc = begin_call(c, k, rw.tab, r->pin_in, head + tabb)) != HNET_OK) return rc;
    if ((rc = enqueue_track(s, reloc_targets_store(s), table_view(rw.tab, n), n, o.track, &rec)) != HNET_OK) return rc;
    if ((rc = finish_call(c, k, rw.rout, r->pin_out, out, (size_t)n * sizeof(RecoverRec))) != HNET_OK) return rc;
    for (int i = 0; i < n; i++) {
        k->has_key[ids[i]] = 1;
        k->count_at_track[ids[i]] = s->st[ids[i]].count;
    }
    return HNET_OK;
}

double hnet_sessions_last_keyframe_device_ms(hnet_sessions* s) { return s && s->kf ? s->kf->ms : 0.0; }

}  // extern "C"
