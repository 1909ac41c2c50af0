// capi_filters.hip — hnet_filters_* and hnet_filter_default_* of include/hnet.h: one device filter per session of a sessions object (sessions_internal.h).
// hnet_filters_step and hnet_filters_advance differ in how a call's states get their readings (the host's windows / the device's IMU rings and the
// initialiser); the IEKF iterations of an attempt, the overflow test and the bookkeeping of an accepted call are one piece of code each, below.
// The two features that add a measurement behind the network's iterations - the photometric fallback (filters_enqueue_refine) and the keyframe
// measurement with or without recovery (filters_enqueue_keyframe, ONE path: the track is capi_keyframe.hip's keyframes_instep_track, the measure and
// finish kernels kernels_filters_keyframe.hip's) - share the filter's own launches on it (filters_enqueue_measured).  The sections of every
// scratch block are carved by capi_internal.h's Carver.
#include "sessions_internal.h"
#include "filters_refine_dev.h"
#include "filters_keyframe_dev.h"

using namespace hnet;
using namespace capi;

// a launch with an opt-in device time: its two events are recorded only once the caller has asked for the time (`timed`); ms: the last timed launch's
struct TimedLaunch { hipEvent_t ev0 = nullptr, ev1 = nullptr; bool timed = false; double ms = NAN; };

// ---- filters: one 27-state filter per session of a sessions object (include/hnet.h).  Device: the states [n_sessions], the parameters [n_sessions] and
// the step's buffers sized for max_batch; host: each state's time (the t_frame check) and camera-IMU offset (the selection window).  A step works on a
// copy of the listed states (work) and scatters it back only once its forwards are accepted: an overflow / timeout repeat starts from the untouched states.
struct hnet_filters {
    hnet_sessions* s = nullptr;
    int iters = 1;
    FilterRec* d_state = nullptr;              // [n_sessions]
    FilterParams* d_params = nullptr;          // [n_sessions]
    std::vector<double> t, cam_imu_dt;         // host mirror of state t / the offset of each session
    std::vector<int> imu_avg;
    // step outputs, ONE device block {net [iters][B][72] f32 | prior_px [iters][B][8] f32 | updates [B] i32 | work [B] FilterRec} and its pinned copy
    uint8_t* d_out = nullptr;
    uint8_t* pin_out = nullptr;
    size_t off_prior = 0, off_upd = 0, off_work = 0, out_bytes = 0;
    double* d_prior_cam = nullptr;             // [B][8]
    // step inputs, ONE pinned block and its device copy (grown on demand): {readings [R] | t_frame [n] | seq [iters][n] | ids [n] | gate [n] | pairs [n][2] | rd_off [n + 1]}
    uint8_t* pin_in = nullptr;
    uint8_t* d_in = nullptr;
    size_t in_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hnet_timing timing = {};
    int last_n = 0;                            // sessions of the last accepted step (hnet_filters_last_priors)
    // ---- the IMU feed (hnet_filters_enable_feed): per session a device ring of `cap` readings, its head / count mirrored here, the newest reading's time,
    // whether the filter has a state (set_state or the initialiser) and, while it has none, the stamp of the last frame the initialiser dropped
    int cap = 0;
    hnet_ekf::ImuData* d_ring = nullptr;       // [n_sessions][cap]
    ImuRingMeta* d_meta = nullptr;             // [n_sessions]
    InitParams* d_ip = nullptr;                // [n_sessions]
    hnet_ekf::ImuData* d_sel = nullptr;        // [B][2 (cap + 2)]: filter_select_kernel's span and selection
    std::vector<ImuRingMeta> meta;
    std::vector<double> imu_newest, t_seen;
    std::vector<uint8_t> inited;
    std::vector<hnet_init_params> ip;
    std::vector<int> last_slot;                // session -> its workgroup in the last advance, -1 if none (hnet_filters_last_selection)
    // feed_imu: ONE pinned block {segments [n] | readings} and its device copy (grown on demand); ev_feed: the pinned block's last upload
    uint8_t* pin_feed = nullptr;
    uint8_t* d_feed = nullptr;
    size_t feed_cap = 0;
    hipEvent_t ev_feed = nullptr;
    // advance: ONE pinned block {jobs [B] | seq [iters][B] | gate [B] | ids [B] | pairs [B][2]} and its device copy; the results [B] behind the step's output block
    uint8_t* pin_adv = nullptr;
    uint8_t* d_adv = nullptr;
    size_t off_res = 0;
    // predict (hnet_filters_predict), allocated by its first call: ONE block {jobs [B] | records [B]}, its pinned copy, and the kernel's own scratch
    uint8_t* pin_pred = nullptr;
    uint8_t* d_pred = nullptr;
    hnet_ekf::ImuData* d_pred_sel = nullptr;   // [B][2 (cap + 2)]
    size_t off_pred_out = 0;
    TimedLaunch pred_time;                     // hnet_filters_last_predict_device_ms
    // predict_cov (hnet_filters_predict_cov), allocated by its first call: ONE block {jobs [B] | records [n] | covariance records [n] | full [n][729]} (the
    // three output sections dense for the call's n, so that one copy downloads what was asked for) and its pinned copy; the scratch is the predict's
    uint8_t* pin_pcov = nullptr;
    uint8_t* d_pcov = nullptr;
    size_t off_pcov_out = 0;
    TimedLaunch pcov_time;                     // hnet_filters_last_predict_cov_device_ms
    // innovations (hnet_filters_enable_innovations): the output block then is {net | prior_px | updates | innov [iters][n] InnovRec, dense | work | results},
    // so that the records lie inside the one download; the per-session gates; the statistics, accumulated from the records of accepted steps
    bool innov = false;
    size_t off_innov = 0;
    double* d_max_nis = nullptr;               // [n_sessions], 0 = no gate
    std::vector<hnet_innovation_stats> innov_stats;
    int last_innov_n = 0;                      // sessions the last accepted step has records for; 0: it ran with innovations off
    // photometric residual records (hnet_filters_enable_photometric): the output block then also holds {photo [n][2 + iters] PhotoRec, dense} behind the
    // innovation records (if any), inside the one download; the slice partials of kernels_photo.hip are device scratch
    bool photo = false;
    size_t off_photo = 0;
    PhotoRec* d_photo_part = nullptr;          // [B][2 + iters][PHOTO_SLICES]
    int last_photo_n = 0;                      // as last_innov_n
    // the photometric gate (hnet_filters_set_photo_gate): the per-session gates on the device and their host mirror (which decides whether a call
    // forms its records per iteration), the per-slot verdict words of photo_gate_kernel, the statistics, where the single-candidate launch takes its taps from
    PhotoGate* d_photo_gate = nullptr;         // [n_sessions], max_ratio 0 = no gate
    int32_t* d_photo_verdict = nullptr;        // [B]
    std::vector<PhotoGate> photo_gate;
    std::vector<hnet_photo_stats> photo_stats;
    bool photo_taps_global = false;
    // the photometric fallback (hnet_filters_set_photo_refine), allocated by the first call that turns it on: the output block then also holds
    // {refine [n] RefineRec, dense} behind the photometric records; per session the options (host: `align` and `levels` decide a call's launch sequence)
    // and what the kernels read of them; ONE zeroed scratch block for the alignment and the fallback's measurement; the statistics
    bool refine = false;
    size_t off_refine = 0;
    std::vector<hnet_photo_refine_opts> refine_opts;
    std::vector<uint8_t> refine_on;
    RefineCfg* d_refine_cfg = nullptr;         // [n_sessions]
    uint8_t* d_refine_scratch = nullptr;       // RefineScratch
    std::vector<hnet_refine_stats> refine_stats;
    int last_refine_n = 0;                     // sessions the last accepted call has refine records for; 0: it ran without a refining session
    // the keyframe track as an in-step measurement (hnet_filters_set_keyframe_measure), allocated by the first call that turns it on: the output
    // block then also holds {kfm [n] KfmRec, dense} behind the refine records; per session the options (host: `track` decides a call's launch sequence)
    // and what the kernels read of them; ONE zeroed scratch block (KfmScratch: the gathered frames, the measurement, the working copies of the keyframe
    // state table and of the prev_ok words, and the prev_ok words themselves); the statistics
    bool kfm = false;
    size_t off_kfm = 0;
    std::vector<hnet_keyframe_measure_opts> kfm_opts;
    std::vector<uint8_t> kfm_on;
    KfmCfg* d_kfm_cfg = nullptr;               // [n_sessions]
    uint8_t* d_kfm_scratch = nullptr;          // KfmScratch
    std::vector<hnet_keyframe_measure_stats> kfm_stats;
    int last_kfm_n = 0;                        // sessions the last accepted call has measure records for; 0: it ran without a measuring session
    // recovery inside the in-step track (hnet_filters_set_keyframe_recover), allocated by the first call that turns it on: the output block
    // then also holds {kfmr [n] OrientedRelocRec, dense} behind the measure records; per measuring session the reloc options and the table (host: they
    // decide a call's launch sequence; device: every session's table, uploaded when it is set) and ONE zeroed scratch block (KfmrScratch)
    bool kfmr = false;
    size_t off_kfmr = 0;
    std::vector<RelocOpts> kfmr_opts;
    std::vector<SearchHyp> kfmr_tab;           // [n_sessions][SEARCH_MAX_HYP], zero behind a session's entries
    std::vector<int> kfmr_n_hyp;
    std::vector<uint8_t> kfmr_on;
    uint8_t* d_kfmr_scratch = nullptr;         // KfmrScratch
    int last_kfmr_n = 0;                       // sessions the last accepted call has relocalise records for; 0: it ran without a recovering session
};
// the sections of d_refine_scratch for max_batch B and N sessions
struct RefineScratch {
    RobustRec* rec; RobustStart* start; RobustWork* work; RobustSums* part; float *x0, *prior_px, *m72; InnovRec* innov; double* nis0; size_t bytes;
    RefineScratch(uint8_t* b, int B, int N) {
        Carver cv{b};
        rec = cv.take<RobustRec>((size_t)HNET_ALIGN_MAX_LEVELS * B);
        start = cv.take<RobustStart>((size_t)B);
        work = cv.take<RobustWork>((size_t)B);
        part = cv.take<RobustSums>((size_t)B * PHOTO_SLICES);
        x0 = cv.take<float>((size_t)B * 8);
        prior_px = cv.take<float>((size_t)B * 8);
        m72 = cv.take<float>((size_t)B * 72);
        innov = cv.take<InnovRec>((size_t)B);
        nis0 = cv.take<double>((size_t)N);      // stays zero: "no NIS gate" for a filters object without innovations
        bytes = cv.used;
    }
};

// the sections of d_kfm_scratch for max_batch B and N sessions
struct KfmScratch {
    uint8_t *prev, *curr; float *step, *prior_px, *m72; InnovRec* innov; int32_t *opened, *prev_ok, *prev_ok_work; KeyState* state_work; double* nis0; size_t bytes;
    KfmScratch(uint8_t* b, int B, int N) {
        Carver cv{b};
        prev = cv.take((size_t)B * NPIX);
        curr = cv.take((size_t)B * NPIX);
        step = cv.take<float>((size_t)B * 8);
        prior_px = cv.take<float>((size_t)B * 8);
        m72 = cv.take<float>((size_t)B * 72);
        innov = cv.take<InnovRec>((size_t)B);
        opened = cv.take<int32_t>((size_t)B);
        prev_ok = cv.take<int32_t>((size_t)N);      // starts zero: never measured
        prev_ok_work = cv.take<int32_t>((size_t)N);
        state_work = cv.take<KeyState>((size_t)N);
        nis0 = cv.take<double>((size_t)N);           // stays zero: "no NIS gate" for a filters object without innovations
        bytes = cv.used;
    }
};
// the sections of d_kfmr_scratch for max_batch B and N sessions: the per-session recover_on words (start zero: off) and tables, the per-slot trials the
// track's alignment accepted
struct KfmrScratch {
    int32_t *on, *accepted; SearchHyp* hyps; size_t bytes;
    KfmrScratch(uint8_t* b, int B, int N) {
        Carver cv{b};
        on = cv.take<int32_t>((size_t)N);
        accepted = cv.take<int32_t>((size_t)B);
        hyps = cv.take<SearchHyp>((size_t)N * SEARCH_MAX_HYP);
        bytes = cv.used;
    }
};
// a call's keyframe measurement: the session whose track options serve it (-1: the call has no measuring session), the {ids | curr slot | gap}
// sections of the track's table on the device, and the session whose reloc options and table serve the call's recovery (-1: no stepping session recovers)
struct KfmCall { int ref; const int32_t* d_tab; int rref; };

static size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// grows a pinned block and its device copy to `want` bytes; the stream is drained first (enqueued work may still read either)
static int grow_block(hnet_ctx* c, uint8_t** pin, uint8_t** dev, size_t* cap, size_t want) {
    if (*cap >= want) return HNET_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (*pin) HIPCHK(c, hipHostFree(*pin));
    if (*dev) HIPCHK(c, hipFree(*dev));
    *pin = *dev = nullptr;
    *cap = 0;
    HIPCHK(c, hipHostMalloc((void**)pin, want, hipHostMallocDefault));
    HIPCHK(c, hipMalloc((void**)dev, want));
    *cap = want;
    return HNET_OK;
}
// free and forget: what a failed enable / first call gives back is what hnet_destroy_filters gives back
template <typename T> static void drop_dev(T*& p) { if (p) (void)hipFree((void*)p); p = nullptr; }
static void drop_pin(uint8_t*& p) { if (p) (void)hipHostFree(p); p = nullptr; }
static void drop_event(hipEvent_t& e) { if (e) (void)hipEventDestroy(e); e = nullptr; }
static void drop_timed(TimedLaunch& t) { drop_event(t.ev0); drop_event(t.ev1); }
static void filters_drop_feed(hnet_filters* f) {                  // hnet_filters_enable_feed
    drop_dev(f->d_ring); drop_dev(f->d_meta); drop_dev(f->d_ip); drop_dev(f->d_sel); drop_dev(f->d_adv);
    drop_pin(f->pin_adv);
    drop_event(f->ev_feed);
}
static void filters_drop_predict(hnet_filters* f) {               // predict_buffers
    drop_dev(f->d_pred_sel); drop_dev(f->d_pred);
    drop_pin(f->pin_pred);
    drop_timed(f->pred_time);
}
static void filters_drop_predict_cov(hnet_filters* f) {           // predict_cov_buffers
    drop_dev(f->d_pcov);
    drop_pin(f->pin_pcov);
    drop_timed(f->pcov_time);
}

extern "C" {

// the offsets of the step's output block for max_batch B: {net | prior_px | updates | innov (if enabled) | photo (if enabled) | refine (if on) | kfm (if on) | work | results}
static void filters_out_layout(hnet_filters* f, int B, bool innov, bool photo, bool refine, bool kfm) {
    f->off_prior = al256((size_t)f->iters * B * 72 * sizeof(float));
    f->off_upd = f->off_prior + al256((size_t)f->iters * B * 8 * sizeof(float));
    f->off_innov = f->off_upd + al256((size_t)B * sizeof(int32_t));
    f->off_photo = f->off_innov + (innov ? al256((size_t)f->iters * B * sizeof(InnovRec)) : 0);
    f->off_refine = f->off_photo + (photo ? al256((size_t)(2 + f->iters) * B * sizeof(PhotoRec)) : 0);
    f->off_kfm = f->off_refine + (refine ? al256((size_t)B * sizeof(RefineRec)) : 0);
    f->off_kfmr = f->off_kfm + (kfm ? al256((size_t)B * sizeof(KfmRec)) : 0);
    f->off_work = f->off_kfmr + (f->kfmr ? al256((size_t)B * sizeof(OrientedRelocRec)) : 0);      // (the relocalise records: once recovery was turned on)
    f->off_res = f->off_work + al256((size_t)B * sizeof(FilterRec));
    f->out_bytes = f->off_res + (size_t)B * sizeof(AdvanceResult);
}
// the sections of the output block as typed pointers, on the device (d) and in the pinned copy (h)
struct OutView { float *net, *prior; int32_t* upd; InnovRec* innov; PhotoRec* photo; RefineRec* refine; KfmRec* kfm; FilterRec* work; AdvanceResult* res; OrientedRelocRec* kfmr; };
struct OutViews { OutView d, h; };
static OutView filters_out_view(const hnet_filters* f, uint8_t* b) {
    return OutView{reinterpret_cast<float*>(b), reinterpret_cast<float*>(b + f->off_prior), reinterpret_cast<int32_t*>(b + f->off_upd), reinterpret_cast<InnovRec*>(b + f->off_innov),
                   reinterpret_cast<PhotoRec*>(b + f->off_photo), reinterpret_cast<RefineRec*>(b + f->off_refine), reinterpret_cast<KfmRec*>(b + f->off_kfm), reinterpret_cast<FilterRec*>(b + f->off_work), reinterpret_cast<AdvanceResult*>(b + f->off_res),
                   reinterpret_cast<OrientedRelocRec*>(b + f->off_kfmr)};
}
static OutViews filters_out_views(const hnet_filters* f) { return OutViews{filters_out_view(f, f->d_out), filters_out_view(f, f->pin_out)}; }
// what a step of n stepping sessions downloads in one copy from the start of the output block when the states are not wanted: up to the last record section in use
static size_t filters_down_head(const hnet_filters* f, int n, bool refining, bool measuring, bool recovering) {
    if (recovering) return f->off_kfmr + (size_t)n * sizeof(OrientedRelocRec);
    if (measuring) return f->off_kfm + (size_t)n * sizeof(KfmRec);
    if (refining) return f->off_refine + (size_t)n * sizeof(RefineRec);
    if (f->photo) return f->off_photo + (size_t)n * (2 + f->iters) * sizeof(PhotoRec);
    if (f->innov) return f->off_innov + (size_t)f->iters * n * sizeof(InnovRec);
    return f->off_upd + (size_t)n * sizeof(int32_t);
}
// (photometric enabled) the records of the step's n pairs in the context's staging: candidates zero | prior of iteration 0 | packed mean of every forward
static hipError_t filters_launch_photo(hnet_filters* f, const OutView& d, int n, hipStream_t st) {
    hnet_ctx* c = f->s->ctx;
    const PhotoCands cands{nullptr, d.prior, d.net, (size_t)c->cfg.max_batch * 72};
    return launch_photo_residual((const uint8_t*)c->stage_prev, (const uint8_t*)c->stage_curr, n, cands, 2 + f->iters, f->d_photo_part, d.photo, nullptr, st);
}
// after an accepted step with innovations on: the records [iters][n] of the sessions ids[0 .. n) go into their statistics
static void filters_count_innovations(hnet_filters* f, int n, const int32_t* ids) {
    const InnovRec* rec = filters_out_view(f, f->pin_out).innov;
    for (int it = 0; it < f->iters; it++)
        for (int j = 0; j < n; j++) {
            const InnovRec& r = rec[(size_t)it * n + j];
            hnet_innovation_stats& a = f->innov_stats[ids[j]];
            if (r.flag == HNET_INNOV_USED) { a.used++; a.sum_nis += r.nis; }
            else if (r.flag == HNET_INNOV_REJECTED) a.rejected++;
            else if (r.flag == HNET_INNOV_SINGULAR) a.singular++;
            if ((r.flag == HNET_INNOV_USED || r.flag == HNET_INNOV_REJECTED) && r.nis > a.max_nis) a.max_nis = r.nis;
        }
}

// whether one of the sessions ids[0 .. n) has a photometric gate: the call then forms its photometric records per iteration (filters_enqueue_iekf)
static bool filters_photo_gated(const hnet_filters* f, int n, const int32_t* ids) {
    if (!f->photo) return false;
    for (int j = 0; j < n; j++)
        if (f->photo_gate[ids[j]].max_ratio > 0.0) return true;
    return false;
}
// whether the call in which the sessions ids[0 .. n) step runs the photometric fallback: 1 when one of them has refinement on and a photometric gate
// (without a gate nothing is ever refused), -1 when two sessions with refinement on differ in `align` or `levels`, else 0.  *ref: a refining session
static int filters_refining(const hnet_filters* f, int n, const int32_t* ids, int* ref) {
    if (!f->refine) return 0;
    int first = -1, refining = 0;
    for (int j = 0; j < n; j++) {
        const int id = ids[j];
        if (!f->refine_on[id]) continue;
        if (first < 0) first = id;
        else if (memcmp(&f->refine_opts[id].align, &f->refine_opts[first].align, sizeof(hnet_photo_robust_opts)) != 0 || f->refine_opts[id].levels != f->refine_opts[first].levels)
            return -1;
        if (f->photo_gate[id].max_ratio > 0.0) refining = 1;
    }
    *ref = first;
    return refining;
}
// after an accepted call with refine records: the records [n] of the sessions ids[0 .. n) go into their statistics (include/hnet.h hnet_refine_stats)
static void filters_count_refine(hnet_filters* f, int n, const int32_t* ids) {
    const RefineRec* rec = filters_out_view(f, f->pin_out).refine;
    for (int j = 0; j < n; j++) {
        const RefineRec& r = rec[j];
        if (!(r.flags & HNET_REFINE_ASKED)) continue;
        hnet_refine_stats& a = f->refine_stats[ids[j]];
        a.asked++;
        if (r.flags & HNET_REFINE_APPLIED) a.applied++;
        if (r.flags & HNET_REFINE_UNUSABLE) a.unusable++;
        if (r.flags & HNET_REFINE_NIS_REJECTED) a.nis_rejected++;
        if ((r.flags & (HNET_REFINE_APPLIED | HNET_REFINE_NIS_REJECTED)) && std::isfinite(r.nis)) {
            a.sum_nis += r.nis;
            if (r.nis > a.max_nis) a.max_nis = r.nis;
        }
    }
}
// whether the call in which the sessions ids[0 .. n) step runs the keyframe measurement: 1 when one of them has it on (*ref: such a session), -1 when two
// of them differ in the track's options, -2 when one of the n sessions has refinement on as well (left open: DESIGN 7v), else 0
static int filters_measuring(const hnet_filters* f, int n, const int32_t* ids, int* ref) {
    *ref = -1;
    if (!f->kfm) return 0;
    int first = -1;
    for (int j = 0; j < n; j++) {
        const int id = ids[j];
        if (!f->kfm_on[id]) continue;
        if (first < 0) first = id;
        else if (memcmp(&f->kfm_opts[id].track, &f->kfm_opts[first].track, sizeof(hnet_keyframe_opts)) != 0) return -1;
    }
    if (first < 0) return 0;
    if (f->refine)
        for (int j = 0; j < n; j++)
            if (f->refine_on[ids[j]]) return -2;
    *ref = first;
    return 1;
}
// whether the call in which the sessions ids[0 .. n) step recovers inside its in-step track: 1 when one of them has recovery on (*ref: such a
// session), -1 when two of them differ in the reloc options, -2 when they differ in their tables, else 0
static int filters_recovering(const hnet_filters* f, int n, const int32_t* ids, int* ref) {
    *ref = -1;
    if (!f->kfmr) return 0;
    int first = -1;
    for (int j = 0; j < n; j++) {
        const int id = ids[j];
        if (!f->kfmr_on[id] || !f->kfm_on[id]) continue;
        if (first < 0) first = id;
        else if (memcmp(&f->kfmr_opts[id], &f->kfmr_opts[first], sizeof(RelocOpts)) != 0) return -1;
        else if (f->kfmr_n_hyp[id] != f->kfmr_n_hyp[first] ||
                 memcmp(&f->kfmr_tab[(size_t)id * SEARCH_MAX_HYP], &f->kfmr_tab[(size_t)first * SEARCH_MAX_HYP], (size_t)SEARCH_MAX_HYP * sizeof(SearchHyp)) != 0)
            return -2;
    }
    if (first < 0) return 0;
    *ref = first;
    return 1;
}
static int filters_recovering_refused(hnet_ctx* c, int recovering, const char* who) {
    return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + (recovering == -1 ? ": the recovering sessions differ in the reloc options (hnet_filters_set_keyframe_recover)"
                                                                              : ": the recovering sessions differ in their tables (hnet_filters_set_keyframe_recover)"));
}
static int filters_measuring_refused(hnet_ctx* c, int measuring, const char* who) {
    return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + (measuring == -1 ? ": the sessions with the keyframe measurement on differ in the track's options (hnet_filters_set_keyframe_measure)"
                                                                              : ": sessions with refinement on and sessions with the keyframe measurement on step in one call"));
}
// after an accepted call with measure records: the records [n] of the sessions ids[0 .. n) go into their statistics (include/hnet.h hnet_keyframe_measure_stats)
static void filters_count_kfm(hnet_filters* f, int n, const int32_t* ids) {
    const KfmRec* rec = filters_out_view(f, f->pin_out).kfm;
    for (int j = 0; j < n; j++) {
        const KfmRec& r = rec[j];
        if (!(r.flags & HNET_KFM_ASKED)) continue;
        hnet_keyframe_measure_stats& a = f->kfm_stats[ids[j]];
        a.asked++;
        if (r.flags & HNET_KFM_APPLIED) a.applied++;
        if (r.flags & HNET_KFMR_UNUSABLE) a.unusable++;            // (HNET_KFM_REATTACHED occurs with recovery on only)
        if (r.flags & HNET_KFM_NIS_REJECTED) a.nis_rejected++;
        if ((r.flags & (HNET_KFM_APPLIED | HNET_KFM_NIS_REJECTED)) && std::isfinite(r.nis)) {
            a.sum_nis += r.nis;
            if (r.nis > a.max_nis) a.max_nis = r.nis;
        }
    }
}
// after an accepted call with photometric records: the records [n][2 + iters] of the sessions ids[0 .. n) go into their statistics (include/hnet.h
// hnet_photo_stats).  ref_gate: the reference gates as the call uploaded them (the pinned input block: the device's copy is the one the kernels close).
// An iteration is reached unrejected when no earlier iteration of the step has a photometric rejection, a NIS rejection or a singular S (updates[j] =
// -1 - applied: with nothing skipped before it, `applied` is the iteration that found it).
static void filters_count_photo(hnet_filters* f, int n, const int32_t* ids, const int32_t* ref_gate) {
    const OutView h = filters_out_view(f, f->pin_out);
    const int I = f->iters;
    for (int j = 0; j < n; j++) {
        if (!ref_gate[j]) continue;
        hnet_photo_stats& a = f->photo_stats[ids[j]];
        const PhotoRec* rec = h.photo + (size_t)j * (2 + I);
        const PhotoRec& pr = rec[1];
        for (int it = 0; it < I; it++) {
            const PhotoRec& e = rec[2 + it];
            a.judged++;
            if (e.flags & PHOTO_REJECTED) a.rejected++;
            if (e.flags & PHOTO_DEGENERATE) a.degenerate++;
            if (!((pr.flags | e.flags) & PHOTO_DEGENERATE) && pr.n_inside >= 1 && e.n_inside >= 1) {
                const double ratio = (e.sum_inside / e.n_inside) / (pr.sum_inside / pr.n_inside);
                if (std::isfinite(ratio)) {
                    a.sum_ratio += ratio;
                    if (ratio > a.max_ratio) a.max_ratio = ratio;
                }
            }
            bool stop = (e.flags & PHOTO_REJECTED) != 0 || (h.upd[j] < 0 && -1 - h.upd[j] == it);
            if (f->innov) {
                const int fl = h.innov[(size_t)it * n + j].flag;
                stop = stop || fl == HNET_INNOV_REJECTED || fl == HNET_INNOV_SINGULAR;
            }
            if (stop) break;
        }
    }
}

// the context of forwards 1 .. iters - 1 of a step when the sessions have an iterative model (hnet_sessions_set_iterative_model), else null
static hnet_ctx* filters_iter_ctx(const hnet_filters* f) { return f->iters > 1 ? f->s->iter : nullptr; }
// forward `it` of a step: 0 on the main context ctx[0], later ones on ctx[1] if there is one; both read the pairs gathered into ctx[0]'s staging
static int filters_forward(hnet_ctx* const ctx[2], int it, const FwdArgs& a, hipStream_t st) {
    hnet_ctx* m = it > 0 && ctx[1] ? ctx[1] : ctx[0];
    const int r = forward(m, a, st);
    return r == HNET_OK || m == ctx[0] ? r : fail(ctx[0], r, "iterative model: " + m->err);
}
// the end of a step's attempt: the flag word of every context that ran downloaded and cleared (run_host_call), the one synchronisation
static int filters_flags(hnet_ctx* const ctx[2], uint32_t* flag, hipStream_t st) {
    hnet_ctx* c = ctx[0];
    for (int k = 0; k < 2; k++)
        if (ctx[k]) {
            HIPCHK(c, hipMemcpyAsync(&flag[k], ctx[k]->d_flag, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipMemsetAsync(ctx[k]->d_flag, 0, 4, st));
        }
    HIPCHK(c, hipStreamSynchronize(st));
    return HNET_OK;
}
// the IEKF iterations of one attempt for the first n workgroups of d.work (n = 0: none), whose pairs lie gathered in ctx[0]'s staging: per iteration the
// prior, the forward, the innovation record (if enabled) and the update; then ev1 and, behind it, the photometric records (hnet_filters_last_timing keeps
// its meaning; inside the attempt: a repeat recomputes the records).  d_seq is [iters][seq_stride]; filter_innovation_kernel closes the d_gate entry of a
// session it rejects, so every attempt uploads the gates again.
// photo_gated (one of the n sessions has a photometric gate): the photometric records are formed per iteration instead, between the forward and the
// innovation kernel - photo_iter_kernel and photo_gate_kernel, which closes d_gate and sets the slot's verdict word on a rejection (iteration 0 writes
// every verdict word: a repeat re-forms them) - and nothing runs behind ev1.
// refine_ref >= 0 (filters_refining said 1; photo_gated then holds): the call runs the photometric fallback with the alignment options of session refine_ref.
// The last iteration's update then leaves the reset to the fallback's update launch, and filters_enqueue_refine follows inside the device window.
// kfm.ref >= 0 (filters_measuring said 1; refine_ref is then -1): the call runs the keyframe measurement with the track options of session kfm.ref.  The
// last iteration's update then runs with update_offset = 1 and leaves the reset to the measurement's update launch, and filters_enqueue_keyframe follows
// inside the device window.
static int filters_enqueue_refine(hnet_filters* f, hnet_ctx* c, const OutView& d, int n, const int32_t* d_ids, int32_t* d_gate, int refine_ref, hipStream_t st);
static int filters_enqueue_keyframe(hnet_filters* f, hnet_ctx* c, const OutView& d, int n, const int32_t* d_ids, int32_t* d_gate, const KfmCall& kfm, hipStream_t st);
static int filters_enqueue_iekf(hnet_filters* f, hnet_ctx* const ctx[2], const OutView& d, int n, const int32_t* d_ids, int32_t* d_gate, const uint64_t* d_seq,
                                int seq_stride, bool photo_gated, int refine_ref, const KfmCall& kfm, hipStream_t st) {
    hnet_ctx* c = ctx[0];
    const int I = f->iters, B = c->cfg.max_batch, N = f->s->n;
    for (int it = 0; it < I && n; it++) {
        float* pr_it = d.prior + (size_t)it * B * 8;
        float* net_it = d.net + (size_t)it * B * 72;
        HIPCHK(c, launch_filter_prior(d.work, n, pr_it, f->d_prior_cam, st));
        const FwdArgs a{.prev = c->stage_prev, .curr = c->stage_curr, .prior = c->cfg.use_prior ? pr_it : nullptr, .batch = n, .mean = net_it, .cov = net_it + 8,
                        .seq_tab = d_seq + (size_t)it * seq_stride, .mean_stride = HNET_PACKED_FLOATS, .cov_stride = HNET_PACKED_FLOATS};
        if (const int r = filters_forward(ctx, it, a, st); r != HNET_OK) return r;
        if (photo_gated) {
            const PhotoCands cands{nullptr, d.prior, d.net, (size_t)B * 72};
            HIPCHK(c, launch_photo_iteration((const uint8_t*)c->stage_prev, (const uint8_t*)c->stage_curr, n, cands, it, I, !f->photo_taps_global, f->d_photo_part,
                                             d_ids, N, f->d_photo_gate, d.upd, d_gate, f->d_photo_verdict, d.photo, st));
        }
        if (f->innov)
            HIPCHK(c, launch_filter_innovation(d_ids, n, N, f->d_params, d.work, net_it, f->d_prior_cam, f->d_max_nis, d_gate, d.upd, it, d.innov,
                                               photo_gated ? f->d_photo_verdict : nullptr, st));
        HIPCHK(c, launch_filter_update(d_ids, n, N, f->d_params, net_it, f->d_prior_cam, d_gate, it != I - 1 || kfm.ref >= 0, it == I - 1 && refine_ref < 0 && kfm.ref < 0,
                                       d.work, d.upd, st));
    }
    if (refine_ref >= 0 && n)
        if (const int r = filters_enqueue_refine(f, c, d, n, d_ids, d_gate, refine_ref, st); r != HNET_OK) return r;
    if (kfm.ref >= 0 && n)
        if (const int r = filters_enqueue_keyframe(f, c, d, n, d_ids, d_gate, kfm, st); r != HNET_OK) return r;
    HIPCHK(c, hipEventRecord(f->ev1, st));
    if (f->photo && n && !photo_gated) HIPCHK(c, filters_launch_photo(f, d, n, st));
    return HNET_OK;
}
// The filter's own launches on a feature's packed measurement m72 [n][72], behind the feature's measure kernel (which opened d_gate for the usable slots
// and closed it for every other): the prior into the feature's prior_px, the innovation record into the feature's innov under the sessions' NIS gates
// (nis0: zeros, for a filters object without innovations), and the update with update_offset = 0 and last = 1: the reset every slot is still owed.
static int filters_enqueue_measured(hnet_filters* f, hnet_ctx* c, const OutView& d, int n, const int32_t* d_ids, int32_t* d_gate, float* prior_px, const float* m72,
                                    const double* nis0, InnovRec* innov, hipStream_t st) {
    const int N = f->s->n;
    HIPCHK(c, launch_filter_prior(d.work, n, prior_px, f->d_prior_cam, st));
    HIPCHK(c, launch_filter_innovation(d_ids, n, N, f->d_params, d.work, m72, f->d_prior_cam, f->innov ? f->d_max_nis : nis0, d_gate, d.upd, 0, innov, nullptr, st));
    HIPCHK(c, launch_filter_update(d_ids, n, N, f->d_params, m72, f->d_prior_cam, d_gate, 0, 1, d.work, d.upd, st));
    return HNET_OK;
}
// The fallback of a call's n stepping sessions, behind the last iteration's update (which ran with last = 0): which slots align (verdict 1, refinement
// on, nothing applied) from iteration 0's fp32 prior, the alignment on the staged pairs (NaN starts elsewhere: DEGENERATE at every level, early returns),
// the measurement (it opens d_gate for the usable slots and closes it for every other), then the filter's own prior, innovation and update launches on
// it - the update with update_offset = 0 and last = 1: the reset every slot is still owed - and what became of it.
static int filters_enqueue_refine(hnet_filters* f, hnet_ctx* c, const OutView& d, int n, const int32_t* d_ids, int32_t* d_gate, int refine_ref, hipStream_t st) {
    const int B = c->cfg.max_batch, N = f->s->n;
    const RefineScratch w(f->d_refine_scratch, B, N);
    const hnet_photo_refine_opts& ro = f->refine_opts[refine_ref];
    RobustOpts o;
    memcpy(&o, &ro.align, sizeof o);
    const size_t pyr = (size_t)B * PYR_BYTES;
    HIPCHK(c, launch_filter_refine_select(d_ids, n, N, f->d_refine_cfg, f->d_photo_verdict, d.upd, d.prior, w.x0, d.refine, st));
    HIPCHK(c, launch_photo_align_robust((const uint8_t*)c->stage_prev, (const uint8_t*)c->stage_curr, n, w.x0, o, ro.levels, c->pyr_scratch, c->pyr_scratch + pyr, w.start,
                                        w.part, w.work, w.rec, st));
    HIPCHK(c, launch_filter_refine_measure(d_ids, n, N, f->d_params, f->d_refine_cfg, w.rec, ro.levels, w.m72, d_gate, d.refine, st));
    if (const int r = filters_enqueue_measured(f, c, d, n, d_ids, d_gate, w.prior_px, w.m72, w.nis0, w.innov, st); r != HNET_OK) return r;
    HIPCHK(c, launch_filter_refine_finish(n, w.innov, d.upd, f->iters, d.refine, st));
    return HNET_OK;
}
// The keyframe measurement of a call's n stepping sessions, behind the last iteration's update (which ran with update_offset = 1 and last = 0): the
// filter's step into the track's table, the track's launches up to decide (capi_keyframe.hip: the keyframe gathered into the feature's own buffers,
// decide on a working copy of the state table; slots that do not measure carry id -1 and NaN steps: early returns), the measurement (it opens d_gate
// for the usable selected slots and closes it for every other), then the filter's own prior, innovation and update launches on it - the update with
// update_offset = 0 and last = 1: the reset every slot is still owed - and what became of it.  Nothing here writes the keyframe store, the map or the
// prev_ok words: filters_commit_keyframe does, once the attempt is accepted.
static int filters_enqueue_keyframe(hnet_filters* f, hnet_ctx* c, const OutView& d, int n, const int32_t* d_ids, int32_t* d_gate, const KfmCall& kfm, hipStream_t st) {
    const int B = c->cfg.max_batch, N = f->s->n;
    const KfmScratch w(f->d_kfm_scratch, B, N);
    KeyOpts ko;
    memcpy(&ko, &f->kfm_opts[kfm.ref].track, sizeof ko);
    const KeyTable tab{w.step, kfm.d_tab, kfm.d_tab + n, kfm.d_tab + 2 * (size_t)n};
    const bool recovering = kfm.rref >= 0;                         //  the track with recovery; the measure and finish kernels then read its records
    const KfmrScratch rw(recovering ? f->d_kfmr_scratch : nullptr, B, N);
    capi::KeyRecovery rc{};
    if (recovering) rc = capi::KeyRecovery{f->kfmr_opts[kfm.rref], rw.hyps + (size_t)kfm.rref * SEARCH_MAX_HYP, f->kfmr_n_hyp[kfm.rref], rw.on, rw.accepted};
    capi::KeyInstep v;
    HIPCHK(c, launch_filter_kfm_step(d_ids, n, N, f->d_kfm_cfg, d.work, w.step, d.kfm, st));
    if (const int r = capi::keyframes_instep_track(f->s, tab, n, ko, recovering ? &rc : nullptr, w.prev, w.curr, w.state_work, &v); r != HNET_OK) return r;
    HIPCHK(c, hipMemcpyAsync(w.prev_ok_work, w.prev_ok, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    HIPCHK(c, launch_filter_kfm_measure(d_ids, n, N, f->d_params, f->d_kfm_cfg, v.state, w.prev_ok, v.track, v.rout, rc.accepted, v.rec, v.levels, d.upd,
                                        w.m72, d_gate, w.opened, d.kfm, st));
    if (const int r = filters_enqueue_measured(f, c, d, n, d_ids, d_gate, w.prior_px, w.m72, w.nis0, w.innov, st); r != HNET_OK) return r;
    HIPCHK(c, launch_filter_kfm_finish(d_ids, n, N, w.innov, d.upd, w.opened, f->iters, v.rout, w.prev_ok_work, d.kfm, recovering ? d.kfmr : nullptr, st));
    return HNET_OK;
}
// the tail of an ACCEPTED call with a keyframe measurement, stream ordered behind the attempt and not synchronised: the track's commits (the state
// table, the new keyframes' images, the map's note and store) and the prev_ok words; then the keyframe layer's host mirrors
static int filters_commit_keyframe(hnet_filters* f, hnet_ctx* c, int n, const int32_t* ids, const KfmCall& kfm, hipStream_t st) {
    const int B = c->cfg.max_batch, N = f->s->n;
    const KfmScratch w(f->d_kfm_scratch, B, N);
    const KeyTable tab{w.step, kfm.d_tab, kfm.d_tab + n, kfm.d_tab + 2 * (size_t)n};
    if (const int r = capi::keyframes_instep_commit(f->s, tab, n, kfm.rref >= 0, w.curr, w.state_work); r != HNET_OK) return r;
    HIPCHK(c, hipMemcpyAsync(w.prev_ok, w.prev_ok_work, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    capi::keyframes_instep_accepted(f->s, n, ids, f->kfm_on.data());
    return HNET_OK;
}
// an overflow of the fp16 planes among the downloaded outputs of n stepping sessions: the first forward with a non-finite output had finite inputs (its
// fp32 priors; later priors follow from it).  -> the index in ctx of the context to repair, -1: none
static int filters_overflowed(const hnet_filters* f, hnet_ctx* const ctx[2], const OutView& h, int n) {
    const hnet_ctx* c = ctx[0];
    const size_t B = (size_t)c->cfg.max_batch;
    for (int it = 0; it < f->iters && n; it++)
        if (!all_finite(h.net + it * B * 72, (size_t)n * 72))
            return !c->cfg.use_prior || all_finite(h.prior + it * B * 8, (size_t)n * 8) ? (it > 0 && ctx[1] ? 1 : 0) : -1;
    return -1;
}
// the bookkeeping of an accepted call in which the sessions ids[0 .. n) stepped: what the last_* calls describe, the innovation statistics, the timing
static int filters_accepted(hnet_filters* f, int n, const int32_t* ids, const int32_t* ref_gate, bool refining, bool measuring, bool recovering,
                            std::chrono::steady_clock::time_point t0, int n_inferences) {
    f->last_n = n;
    f->last_innov_n = f->innov ? n : 0;
    f->last_photo_n = f->photo ? n : 0;
    if (f->innov) filters_count_innovations(f, n, ids);
    if (f->photo) filters_count_photo(f, n, ids, ref_gate);
    f->last_refine_n = refining ? n : 0;
    if (refining) filters_count_refine(f, n, ids);
    f->last_kfm_n = measuring ? n : 0;
    if (measuring) filters_count_kfm(f, n, ids);
    f->last_kfmr_n = recovering ? n : 0;
    float ms = 0;
    HIPCHK(f->s->ctx, hipEventElapsedTime(&ms, f->ev0, f->ev1));
    record_timing(f->timing, ms, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), n_inferences, true);
    return HNET_OK;
}

void hnet_filter_default_params(hnet_filter_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    static const double T[12] = {-0.027256691772188965, -0.9996260641688061, 0.0021919370477445077, 0.02422852666805565,
                                 -0.7139206120417471, 0.017931469899155242, -0.6999970157716363, 0.008974432843748055,
                                 0.6996959571525168, -0.020644471939022302, -0.714142404092339, -0.000638971731537894};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) p->c_R_i[i * 3 + j] = T[i * 4 + j];
    for (int i = 0; i < 3; i++) p->i_t_i2c[i] = -(p->c_R_i[i] * T[3] + p->c_R_i[3 + i] * T[7] + p->c_R_i[6 + i] * T[11]);
    p->sigma_w = 0.00559017;
    p->sigma_wb = 8.94427e-04;
    p->sigma_a = 0.01118034;
    p->sigma_ab = 0.04472136;
    p->gravity_mag = 9.81;
    p->k_net_cov = 10.0;
    p->cam_imu_dt = 0.0;
    p->imu_avg = 1;
}

static FilterParams filter_params_dev(const hnet_filter_params& p) {
    FilterParams d;
    memset(&d, 0, sizeof d);
    memcpy(d.ext.c_R_i, p.c_R_i, sizeof d.ext.c_R_i);
    memcpy(d.ext.i_t_i2c, p.i_t_i2c, sizeof d.ext.i_t_i2c);
    hnet_ekf::noise_q_diag(p.sigma_w, p.sigma_a, p.sigma_wb, p.sigma_ab, d.q);
    d.gravity_mag = p.gravity_mag;
    d.k_net_cov = p.k_net_cov;
    d.imu_avg = p.imu_avg ? 1 : 0;
    return d;
}

void hnet_destroy_filters(hnet_filters* f) {
    if (!f) return;
    hnet_ctx* c = f->s->ctx;
    (void)hipSetDevice(c->cfg.device_id);
    (void)hipStreamSynchronize(c->stream);
    drop_dev(f->d_state); drop_dev(f->d_params); drop_dev(f->d_out); drop_dev(f->d_prior_cam); drop_dev(f->d_in); drop_dev(f->d_feed); drop_dev(f->d_max_nis); drop_dev(f->d_photo_part); drop_dev(f->d_photo_gate); drop_dev(f->d_photo_verdict); drop_dev(f->d_refine_cfg); drop_dev(f->d_refine_scratch); drop_dev(f->d_kfm_cfg); drop_dev(f->d_kfm_scratch); drop_dev(f->d_kfmr_scratch);
    drop_pin(f->pin_feed); drop_pin(f->pin_out); drop_pin(f->pin_in);
    drop_event(f->ev0); drop_event(f->ev1);
    filters_drop_feed(f);
    filters_drop_predict(f);
    filters_drop_predict_cov(f);
    delete f;
}

int hnet_create_filters(hnet_sessions* s, int max_iekf_iteration, hnet_filters** out) {
    if (!s || !out) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    if (max_iekf_iteration < 1 || max_iekf_iteration > 64) return fail(c, HNET_ERR_INVALID_ARG, "hnet_create_filters: max_iekf_iteration outside 1 .. 64");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    hnet_filters* f = new hnet_filters();
    f->s = s;
    f->iters = max_iekf_iteration;
    const int N = s->n, B = c->cfg.max_batch;
    hnet_filter_params dp;
    hnet_filter_default_params(&dp);
    f->t.assign(N, 0.0);
    f->cam_imu_dt.assign(N, dp.cam_imu_dt);
    f->imu_avg.assign(N, dp.imu_avg);
    filters_out_layout(f, B, false, false, false, false);
    f->t_seen.assign(N, -INFINITY);
    f->inited.assign(N, 0);
    f->last_slot.assign(N, -1);
    hnet_init_params ip0;
    hnet_filter_default_init_params(&ip0);
    f->ip.assign(N, ip0);
    std::vector<FilterRec> st(N);
    memset(st.data(), 0, st.size() * sizeof(FilterRec));
    for (auto& r : st) r.s.q[0] = 1.0;
    std::vector<FilterParams> pr(N, filter_params_dev(dp));
    hipError_t e = hipMalloc((void**)&f->d_state, (size_t)N * sizeof(FilterRec));
    if (e == hipSuccess) e = hipMalloc((void**)&f->d_params, (size_t)N * sizeof(FilterParams));
    if (e == hipSuccess) e = hipMalloc((void**)&f->d_out, f->out_bytes);
    if (e == hipSuccess) e = hipHostMalloc((void**)&f->pin_out, f->out_bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void**)&f->d_prior_cam, (size_t)B * 8 * sizeof(double));
    if (e == hipSuccess) e = hipEventCreate(&f->ev0);
    if (e == hipSuccess) e = hipEventCreate(&f->ev1);
    if (e == hipSuccess) e = hipMemcpyAsync(f->d_state, st.data(), (size_t)N * sizeof(FilterRec), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(f->d_params, pr.data(), (size_t)N * sizeof(FilterParams), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        hnet_destroy_filters(f);
        return fail(c, HNET_ERR_DEVICE, std::string("hnet_create_filters: ") + hipGetErrorString(e));
    }
    *out = f;
    return HNET_OK;
}

int hnet_filters_set_params(hnet_filters* f, int id, const hnet_filter_params* p) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = f->s->ctx;
    if (!p || id < 0 || id >= f->s->n) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_set_params: id or params");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const FilterParams d = filter_params_dev(*p);
    HIPCHK(c, hipMemcpyAsync(f->d_params + id, &d, sizeof d, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    f->cam_imu_dt[id] = p->cam_imu_dt;
    f->imu_avg[id] = p->imu_avg ? 1 : 0;
    return HNET_OK;
}

static_assert(sizeof(hnet_filter_state) == sizeof(FilterRec), "hnet_filter_state is the FilterRec layout");

int hnet_filters_set_state(hnet_filters* f, int id, const hnet_filter_state* st) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = f->s->ctx;
    if (!st || id < 0 || id >= f->s->n) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_set_state: id or state");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipMemcpyAsync(f->d_state + id, st, sizeof(FilterRec), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    f->t[id] = st->t;
    f->inited[id] = 1;
    return HNET_OK;
}

int hnet_filters_get_state(hnet_filters* f, int n, const int32_t* ids, hnet_filter_state* out) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = f->s->ctx;
    if (!ids || !out || n < 1) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_get_state: ids / out");
    for (int i = 0; i < n; i++)
        if (ids[i] < 0 || ids[i] >= f->s->n) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_get_state: id out of range");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    for (int i = 0; i < n; i++) HIPCHK(c, hipMemcpyAsync(out + i, f->d_state + ids[i], sizeof(FilterRec), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HNET_OK;
}

int hnet_filters_step(hnet_filters* f, int n, const int32_t* ids, const double* t_frame, const hnet_imu* imu, const int64_t* imu_off,
                      hnet_filter_state* state_out, float* net_out, int32_t* updates) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_sessions* s = f->s;
    hnet_ctx* c = s->ctx;
    if (!t_frame || !imu_off) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_step: t_frame / imu_off");
    int rc = sessions_check_ids(s, n, ids);
    if (rc == HNET_OK) rc = sessions_check_pairs(s, n, ids);
    if (rc != HNET_OK) return rc;
    int refine_ref = -1;
    const int refining = filters_refining(f, n, ids, &refine_ref);
    if (refining < 0) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_step: the sessions with refinement on differ in align / levels (hnet_filters_set_photo_refine)");
    if (!refining) refine_ref = -1;
    int kfm_ref = -1;
    const int measuring = filters_measuring(f, n, ids, &kfm_ref);
    if (measuring < 0) return filters_measuring_refused(c, measuring, "hnet_filters_step");
    int kfmr_ref = -1;
    const int recovering = measuring ? filters_recovering(f, n, ids, &kfmr_ref) : 0;
    if (recovering < 0) return filters_recovering_refused(c, recovering, "hnet_filters_step");
    for (int i = 0; i < n; i++) {
        if (!(t_frame[i] > f->t[ids[i]]) || !std::isfinite(t_frame[i]))
            return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_step: t_frame must be later than the state's time (Propagator.cpp:32-43)");
        if (imu_off[i] < 0 || imu_off[i + 1] < imu_off[i] || (imu_off[i + 1] > imu_off[i] && !imu))
            return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_step: imu / imu_off");
    }
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    auto t0 = std::chrono::steady_clock::now();
    const int I = f->iters;
    // selection on the host (hnet_ekf::select_imu_readings: the window [state t, t_frame] + the session's offset) into the input block
    static_assert(sizeof(hnet_imu) == sizeof(hnet_ekf::ImuData), "hnet_imu is hnet_ekf::ImuData");
    int64_t total = 0;
    for (int i = 0; i < n; i++) total += imu_off[i + 1] - imu_off[i] + 2;
    const size_t o_t = al256((size_t)total * sizeof(hnet_ekf::ImuData)), o_seq = o_t + al256((size_t)n * 8), o_ids = o_seq + al256((size_t)I * n * 8);
    const size_t o_gate = o_ids + al256((size_t)n * 4), o_pairs = o_gate + al256((size_t)n * 4), o_off = o_pairs + al256((size_t)n * 8);
    const size_t o_kf = o_off + al256((size_t)(n + 1) * 4);                          // (with a measuring session: the track's {ids | curr slot | gap} behind the rest)
    const size_t in_bytes = o_kf + (measuring ? al256((size_t)n * 12) : 0);
    if ((rc = grow_block(c, &f->pin_in, &f->d_in, &f->in_cap, in_bytes)) != HNET_OK) return rc;
    hnet_ekf::ImuData* rd = reinterpret_cast<hnet_ekf::ImuData*>(f->pin_in);
    double* tf = reinterpret_cast<double*>(f->pin_in + o_t);
    uint64_t* seq = reinterpret_cast<uint64_t*>(f->pin_in + o_seq);
    int32_t* hid = reinterpret_cast<int32_t*>(f->pin_in + o_ids);
    int32_t* gate = reinterpret_cast<int32_t*>(f->pin_in + o_gate);
    int32_t* pairs = reinterpret_cast<int32_t*>(f->pin_in + o_pairs);
    int32_t* roff = reinterpret_cast<int32_t*>(f->pin_in + o_off);
    int R = 0;
    for (int i = 0; i < n; i++) {
        const int id = ids[i];
        const hnet_sessions::Sess& e = s->st[id];
        const int64_t m = imu_off[i + 1] - imu_off[i];
        const double dt = f->cam_imu_dt[id];
        roff[i] = R;
        R += hnet_ekf::select_imu_readings(reinterpret_cast<const hnet_ekf::ImuData*>(imu) + imu_off[i], (int)m, f->t[id] + dt, t_frame[i] + dt, rd + R);
        tf[i] = t_frame[i];
        for (int it = 0; it < I; it++) seq[(size_t)it * n + i] = e.seq + (uint64_t)it;
        hid[i] = id;
        gate[i] = (e.t == t_frame[i] && e.count > 10) ? 1 : 0;                      // VioManager.cpp:257
        sessions_pair(s, id, pairs + 2 * i);
    }
    roff[n] = R;
    if (measuring) capi::keyframes_table(s, n, ids, f->kfm_on.data(), reinterpret_cast<int32_t*>(f->pin_in + o_kf));
    const KfmCall kfm{kfm_ref, reinterpret_cast<const int32_t*>(f->d_in + o_kf), kfmr_ref};
    const hnet_ekf::ImuData* d_rd = reinterpret_cast<const hnet_ekf::ImuData*>(f->d_in);
    const double* d_tf = reinterpret_cast<const double*>(f->d_in + o_t);
    const uint64_t* d_seq = reinterpret_cast<const uint64_t*>(f->d_in + o_seq);
    const int32_t* d_ids = reinterpret_cast<const int32_t*>(f->d_in + o_ids);
    int32_t* d_gate = reinterpret_cast<int32_t*>(f->d_in + o_gate);
    const int32_t* d_pairs = reinterpret_cast<const int32_t*>(f->d_in + o_pairs);
    const int32_t* d_roff = reinterpret_cast<const int32_t*>(f->d_in + o_off);
    const OutViews o = filters_out_views(f);
    // the output block is laid out for max_batch: download the used parts of each section in one copy up to the last one needed
    const size_t down = state_out ? f->off_work + (size_t)n * sizeof(FilterRec) : filters_down_head(f, n, refining > 0, measuring > 0, recovering > 0);
    hipStream_t st = c->stream;
    const size_t up = measuring ? o_kf + (size_t)n * 12 : o_off + (size_t)(n + 1) * 4;
    hnet_ctx* const ctx[2] = {c, filters_iter_ctx(f)};
    const bool photo_gated = filters_photo_gated(f, n, ids);
    auto enqueue = [&](uint32_t* flag_now) -> int {
        HIPCHK(c, hipMemcpyAsync(f->d_in, f->pin_in, up, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemsetAsync(o.d.upd, 0, (size_t)n * sizeof(int32_t), st));
        HIPCHK(c, hipEventRecord(f->ev0, st));
        HIPCHK(c, launch_session_gather(s->ring, 2 * s->n, d_pairs, n, (uint8_t*)c->stage_prev, (uint8_t*)c->stage_curr, st));
        HIPCHK(c, launch_filter_propagate(d_ids, n, s->n, f->d_state, f->d_params, d_rd, d_roff, d_tf, o.d.work, st));
        if (const int r = filters_enqueue_iekf(f, ctx, o.d, n, d_ids, d_gate, d_seq, n, photo_gated, refine_ref, kfm, st); r != HNET_OK) return r;
        HIPCHK(c, hipMemcpyAsync(f->pin_out, f->d_out, down, hipMemcpyDeviceToHost, st));
        return filters_flags(ctx, flag_now, st);
    };
    if ((rc = run_host_call(ctx, enqueue, [&] { return filters_overflowed(f, ctx, o.h, n); })) != HNET_OK) return rc;
    // accepted: the listed states take the step's result (stream order: later calls see it), the bookkeeping advances
    HIPCHK(c, launch_filter_scatter(o.d.work, d_ids, n, s->n, f->d_state, st));
    if (measuring)
        if ((rc = filters_commit_keyframe(f, c, n, ids, kfm, st)) != HNET_OK) return rc;
    for (int i = 0; i < n; i++) {
        f->t[ids[i]] = t_frame[i];
        s->st[ids[i]].seq += (uint64_t)I;
    }
    if (net_out)
        for (int it = 0; it < I; it++) memcpy(net_out + (size_t)it * n * 72, o.h.net + (size_t)it * c->cfg.max_batch * 72, (size_t)n * 72 * sizeof(float));
    if (updates) memcpy(updates, o.h.upd, (size_t)n * sizeof(int32_t));
    if (state_out) memcpy(state_out, o.h.work, (size_t)n * sizeof(FilterRec));
    return filters_accepted(f, n, ids, gate, refining > 0, measuring > 0, recovering > 0, t0, I);
}

int hnet_filters_last_priors(const hnet_filters* f, int n, float* out) {
    if (!f || !out) return HNET_ERR_INVALID_ARG;
    if (f->last_n < 1) return fail(f->s->ctx, HNET_ERR_NOT_READY, "hnet_filters_last_priors: no step yet");
    if (n != f->last_n) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_last_priors: n differs from the last step's");
    const int B = f->s->ctx->cfg.max_batch;
    const float* h_prior = filters_out_view(f, f->pin_out).prior;
    for (int it = 0; it < f->iters; it++) memcpy(out + (size_t)it * f->last_n * 8, h_prior + (size_t)it * B * 8, (size_t)f->last_n * 8 * sizeof(float));
    return HNET_OK;
}

int hnet_filters_last_timing(const hnet_filters* f, hnet_timing* out) {
    if (!f || !out) return HNET_ERR_INVALID_ARG;
    *out = f->timing;
    return HNET_OK;
}

// ---- filters, fed (include/hnet.h): the IMU rings, the initialiser and hnet_filters_advance ----

void hnet_filter_default_init_params(hnet_init_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->window_time = 1.0;
    p->imu_thresh = 0.5;
    p->init_height = 0.1;
    p->wait_for_jerk = 1;
}

static InitParams init_params_dev(const hnet_init_params& p) { return InitParams{p.window_time, p.imu_thresh, p.init_height, p.wait_for_jerk ? 1 : 0, 0}; }
// the advance input block for n sessions: jobs | seq [iters][n] | gate | ids | pairs
struct AdvLayout {
    size_t o_seq, o_gate, o_ids, o_pairs, o_kf, bytes;        // (o_kf: the track's {ids | curr slot | gap} of a call with a measuring session, uploaded only then)
    AdvLayout(int n, int iters) {
        o_seq = al256((size_t)n * sizeof(AdvanceJob));
        o_gate = o_seq + al256((size_t)iters * n * 8);
        o_ids = o_gate + al256((size_t)n * 4);
        o_pairs = o_ids + al256((size_t)n * 4);
        o_kf = o_pairs + al256((size_t)n * 8);
        bytes = o_kf + al256((size_t)n * 12);
    }
};

int hnet_filters_enable_feed(hnet_filters* f, int imu_capacity) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = f->s->ctx;
    if (f->cap) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_enable_feed: already enabled");
    if (imu_capacity < 2 || imu_capacity > (1 << 20)) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_enable_feed: imu_capacity outside 2 .. 1048576");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const int N = f->s->n, B = c->cfg.max_batch;
    const size_t adv = AdvLayout(B, f->iters).bytes;
    std::vector<InitParams> ipd(N);
    for (int i = 0; i < N; i++) ipd[i] = init_params_dev(f->ip[i]);
    hipError_t e = hipMalloc((void**)&f->d_ring, (size_t)N * imu_capacity * sizeof(hnet_ekf::ImuData));
    if (e == hipSuccess) e = hipMalloc((void**)&f->d_meta, (size_t)N * sizeof(ImuRingMeta));
    if (e == hipSuccess) e = hipMalloc((void**)&f->d_ip, (size_t)N * sizeof(InitParams));
    if (e == hipSuccess) e = hipMalloc((void**)&f->d_sel, (size_t)B * 2 * (imu_capacity + 2) * sizeof(hnet_ekf::ImuData));
    if (e == hipSuccess) e = hipMalloc((void**)&f->d_adv, adv);
    if (e == hipSuccess) e = hipHostMalloc((void**)&f->pin_adv, adv, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&f->ev_feed, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMemsetAsync(f->d_meta, 0, (size_t)N * sizeof(ImuRingMeta), c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(f->d_ip, ipd.data(), (size_t)N * sizeof(InitParams), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        filters_drop_feed(f);
        return fail(c, HNET_ERR_DEVICE, std::string("hnet_filters_enable_feed: ") + hipGetErrorString(e));
    }
    f->meta.assign(N, ImuRingMeta{0, 0});
    f->imu_newest.assign(N, -INFINITY);
    f->cap = imu_capacity;
    return HNET_OK;
}

int hnet_filters_set_init_params(hnet_filters* f, int id, const hnet_init_params* p) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = f->s->ctx;
    if (!p || id < 0 || id >= f->s->n || !(p->window_time > 0.0) || !std::isfinite(p->window_time) || !std::isfinite(p->imu_thresh) || !std::isfinite(p->init_height))
        return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_set_init_params: id or params");
    if (f->cap) {
        HIPCHK(c, hipSetDevice(c->cfg.device_id));
        const InitParams d = init_params_dev(*p);
        HIPCHK(c, hipMemcpyAsync(f->d_ip + id, &d, sizeof d, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    f->ip[id] = *p;
    return HNET_OK;
}

int hnet_filters_feed_imu(hnet_filters* f, int n, const int32_t* ids, const hnet_imu* imu, const int64_t* imu_off) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_sessions* s = f->s;
    hnet_ctx* c = s->ctx;
    if (!f->cap) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_feed_imu: feed not enabled (hnet_filters_enable_feed)");
    if (!ids || !imu_off || n < 1 || n > s->n) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_feed_imu: ids / imu_off / n");
    if (imu_off[0] < 0) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_feed_imu: imu_off");
    // validation first: nothing is appended unless every listed session's readings are in order
    int rc = HNET_OK, marked = 0;
    for (int i = 0; i < n && rc == HNET_OK; i++) {
        const int id = ids[i];
        if (id < 0 || id >= s->n) { rc = fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_feed_imu: id out of range"); break; }
        if (s->mark[id]) { rc = fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_feed_imu: id repeated in one call"); break; }
        s->mark[id] = 1;
        marked = i + 1;
        if (imu_off[i + 1] < imu_off[i] || imu_off[i + 1] > INT32_MAX || (imu_off[i + 1] > imu_off[i] && !imu)) { rc = fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_feed_imu: imu / imu_off"); break; }
        double last = f->imu_newest[id];
        for (int64_t k = imu_off[i]; k < imu_off[i + 1]; k++) {
            if (!std::isfinite(imu[k].t) || imu[k].t < last) { rc = fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_feed_imu: readings must be finite and in non-decreasing time"); break; }
            last = imu[k].t;
        }
    }
    for (int j = 0; j < marked; j++) s->mark[ids[j]] = 0;
    if (rc != HNET_OK) return rc;
    const int64_t base = imu_off[0], total = imu_off[n] - base;
    if (total == 0) return HNET_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const size_t o_rd = al256((size_t)n * sizeof(ImuFeedSeg)), bytes = o_rd + (size_t)total * sizeof(hnet_ekf::ImuData);
    HIPCHK(c, hipEventSynchronize(f->ev_feed));                    // the pinned block's last upload has left it
    if (rc = grow_block(c, &f->pin_feed, &f->d_feed, &f->feed_cap, std::max(bytes, (size_t)1 << 16)); rc != HNET_OK) return rc;
    static_assert(sizeof(hnet_imu) == sizeof(hnet_ekf::ImuData), "hnet_imu is hnet_ekf::ImuData");
    ImuFeedSeg* seg = reinterpret_cast<ImuFeedSeg*>(f->pin_feed);
    memcpy(f->pin_feed + o_rd, imu + base, (size_t)total * sizeof(hnet_imu));
    std::vector<ImuRingMeta> next(n);
    int longest = 0;
    for (int i = 0; i < n; i++) {
        const ImuRingMeta m = f->meta[ids[i]];
        const int64_t have = imu_off[i + 1] - imu_off[i];
        const int take = (int)std::min<int64_t>(have, f->cap);      // more than a ring's worth: only the newest `cap` can stay
        const int count = std::min(f->cap, m.count + take);
        const int head = (int)(((int64_t)m.head + m.count + take - count) % f->cap);
        next[i] = ImuRingMeta{head, count};
        seg[i] = ImuFeedSeg{ids[i], (int32_t)(imu_off[i] - base + (have - take)), take, (int32_t)(((int64_t)m.head + m.count) % f->cap), head, count};
        longest = std::max(longest, take);
    }
    HIPCHK(c, hipMemcpyAsync(f->d_feed, f->pin_feed, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(f->ev_feed, c->stream));
    HIPCHK(c, launch_imu_append(reinterpret_cast<const ImuFeedSeg*>(f->d_feed), n, longest, reinterpret_cast<const hnet_ekf::ImuData*>(f->d_feed + o_rd), (int)total,
                                s->n, f->cap, f->d_ring, f->d_meta, c->stream));
    for (int i = 0; i < n; i++) {
        f->meta[ids[i]] = next[i];
        if (imu_off[i + 1] > imu_off[i]) f->imu_newest[ids[i]] = imu[imu_off[i + 1] - 1].t;
    }
    return HNET_OK;
}

int hnet_filters_initialized(const hnet_filters* f, int id) { return (f && id >= 0 && id < f->s->n) ? (int)f->inited[id] : -1; }

int hnet_filters_uninitialize(hnet_filters* f, int id) {
    if (!f) return HNET_ERR_INVALID_ARG;
    if (id < 0 || id >= f->s->n) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_uninitialize: id out of range");
    f->inited[id] = 0;
    f->t_seen[id] = -INFINITY;
    return hnet_sessions_reset(f->s, id);
}

int hnet_filters_advance(hnet_filters* f, int n, const int32_t* ids, hnet_filter_state* state_out, float* net_out, int32_t* updates, int32_t* status) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_sessions* s = f->s;
    hnet_ctx* c = s->ctx;
    if (!f->cap) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_advance: feed not enabled (hnet_filters_enable_feed)");
    if (!status) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_advance: status");
    int rc = sessions_check_ids(s, n, ids);
    if (rc != HNET_OK) return rc;
    auto t_begin = std::chrono::steady_clock::now();
    const int I = f->iters, B = c->cfg.max_batch;
    // what each listed session does (VioManager.cpp:122-162); the sessions that step come first on the device, the propagate-only ones behind them
    std::vector<int> order;                                        // listed index of workgroup j
    order.reserve(n);
    for (int pass = 0; pass < 2; pass++)
        for (int i = 0; i < n; i++) {
            const int id = ids[i];
            const hnet_sessions::Sess& e = s->st[id];
            int st;
            if (e.count < 1 || !(e.t_push > (f->inited[id] ? f->t[id] : f->t_seen[id]))) st = HNET_ADV_NO_FRAME;
            else if (!(e.t_push < f->imu_newest[id] - f->cam_imu_dt[id])) st = HNET_ADV_WAIT_IMU;
            else if (!f->inited[id]) st = HNET_ADV_WAIT_INIT;      // (INITIALIZED if the device's initialiser accepts)
            else st = e.count < 2 ? HNET_ADV_PROPAGATED : HNET_ADV_STEPPED;
            if (pass == 0) status[i] = st;
            if ((pass == 0 && st == HNET_ADV_STEPPED) || (pass == 1 && (st == HNET_ADV_PROPAGATED || st == HNET_ADV_WAIT_INIT))) order.push_back(i);
        }
    const int n_a = (int)order.size();
    int n_s = 0;
    for (int i = 0; i < n; i++) n_s += status[i] == HNET_ADV_STEPPED;
    std::vector<int32_t> stepping(n_s);
    for (int j = 0; j < n_s; j++) stepping[j] = ids[order[j]];
    int refine_ref = -1;
    const int refining = filters_refining(f, n_s, stepping.data(), &refine_ref);
    if (refining < 0) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_advance: the sessions with refinement on differ in align / levels (hnet_filters_set_photo_refine)");
    if (!refining) refine_ref = -1;
    int kfm_ref = -1;
    const int measuring = filters_measuring(f, n_s, stepping.data(), &kfm_ref);
    if (measuring < 0) return filters_measuring_refused(c, measuring, "hnet_filters_advance");
    int kfmr_ref = -1;
    const int recovering = measuring ? filters_recovering(f, n_s, stepping.data(), &kfmr_ref) : 0;
    if (recovering < 0) return filters_recovering_refused(c, recovering, "hnet_filters_advance");
    if (net_out) memset(net_out, 0, (size_t)I * n * 72 * sizeof(float));
    if (updates) memset(updates, 0, (size_t)n * sizeof(int32_t));
    std::fill(f->last_slot.begin(), f->last_slot.end(), -1);
    f->last_photo_n = 0;                                           // (a call in which nothing steps has no photometric records, whatever the call before it left)
    f->last_refine_n = 0;
    f->last_kfm_n = 0;
    f->last_kfmr_n = 0;
    if (n_a == 0) return HNET_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const AdvLayout L(n_a, I);
    AdvanceJob* job = reinterpret_cast<AdvanceJob*>(f->pin_adv);
    uint64_t* seq = reinterpret_cast<uint64_t*>(f->pin_adv + L.o_seq);
    int32_t* gate = reinterpret_cast<int32_t*>(f->pin_adv + L.o_gate);
    int32_t* hid = reinterpret_cast<int32_t*>(f->pin_adv + L.o_ids);
    int32_t* pairs = reinterpret_cast<int32_t*>(f->pin_adv + L.o_pairs);
    bool any_init = false;
    for (int j = 0; j < n_a; j++) {
        const int i = order[j], id = ids[i];
        const hnet_sessions::Sess& e = s->st[id];
        const bool init = status[i] == HNET_ADV_WAIT_INIT;
        any_init |= init;
        job[j] = AdvanceJob{e.t_push, f->cam_imu_dt[id], id, init ? 1 : 0, j >= n_s ? 1 : 0, 0};
        for (int it = 0; it < I; it++) seq[(size_t)it * n_a + j] = e.seq + (uint64_t)it;
        gate[j] = (j < n_s && e.t == e.t_push && e.count > 10) ? 1 : 0;             // VioManager.cpp:257
        hid[j] = id;
        sessions_pair(s, id, pairs + 2 * j);
    }
    if (measuring) capi::keyframes_table(s, n_s, stepping.data(), f->kfm_on.data(), reinterpret_cast<int32_t*>(f->pin_adv + L.o_kf));
    const KfmCall kfm{kfm_ref, reinterpret_cast<const int32_t*>(f->d_adv + L.o_kf), kfmr_ref};
    const AdvanceJob* d_job = reinterpret_cast<const AdvanceJob*>(f->d_adv);
    const uint64_t* d_seq = reinterpret_cast<const uint64_t*>(f->d_adv + L.o_seq);
    int32_t* d_gate = reinterpret_cast<int32_t*>(f->d_adv + L.o_gate);
    const int32_t* d_ids = reinterpret_cast<const int32_t*>(f->d_adv + L.o_ids);
    const int32_t* d_pairs = reinterpret_cast<const int32_t*>(f->d_adv + L.o_pairs);
    const OutViews o = filters_out_views(f);
    FilterRec* d_work = o.d.work;
    AdvanceResult* d_res = o.d.res;
    hipStream_t st = c->stream;
    hnet_ctx* const ctx[2] = {c, n_s ? filters_iter_ctx(f) : nullptr};
    const bool photo_gated = filters_photo_gated(f, n_s, hid);
    auto enqueue = [&](uint32_t* flag_now) -> int {
        HIPCHK(c, hipMemcpyAsync(f->d_adv, f->pin_adv, measuring ? L.o_kf + (size_t)n_s * 12 : L.o_kf, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemsetAsync(o.d.upd, 0, (size_t)n_a * sizeof(int32_t), st));
        HIPCHK(c, hipEventRecord(f->ev0, st));
        if (any_init)                                              // (the sessions without a state are among the propagate-only ones)
            HIPCHK(c, launch_filter_init(d_job + n_s, n_a - n_s, s->n, f->cap, f->d_ring, f->d_meta, f->d_ip, f->d_params, d_work + n_s, d_res + n_s, st));
        HIPCHK(c, launch_filter_select(d_job, n_a, s->n, f->cap, f->d_ring, f->d_meta, f->d_state, d_work, f->d_sel, d_res, st));
        if (n_s) HIPCHK(c, launch_session_gather(s->ring, 2 * s->n, d_pairs, n_s, (uint8_t*)c->stage_prev, (uint8_t*)c->stage_curr, st));
        HIPCHK(c, launch_filter_propagate_adv(d_job, n_a, s->n, f->cap, f->d_state, f->d_params, f->d_sel, d_res, d_work, st));
        if (const int r = filters_enqueue_iekf(f, ctx, o.d, n_s, d_ids, d_gate, d_seq, n_a, photo_gated, refine_ref, kfm, st); r != HNET_OK) return r;     // (the sequence table has a row of n_a per iteration)
        if (n_s) HIPCHK(c, hipMemcpyAsync(f->pin_out, f->d_out, filters_down_head(f, n_s, refining > 0, measuring > 0, recovering > 0), hipMemcpyDeviceToHost, st));
        if (state_out) HIPCHK(c, hipMemcpyAsync(f->pin_out + f->off_work, d_work, (size_t)n_a * sizeof(FilterRec), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(f->pin_out + f->off_res, d_res, (size_t)n_a * sizeof(AdvanceResult), hipMemcpyDeviceToHost, st));
        return filters_flags(ctx, flag_now, st);
    };
    if ((rc = run_host_call(ctx, enqueue, [&] { return filters_overflowed(f, ctx, o.h, n_s); })) != HNET_OK) return rc;
    // accepted: the states take the results (not those the initialiser refused), the bookkeeping advances
    HIPCHK(c, launch_filter_scatter_ok(d_work, d_job, d_res, n_a, s->n, f->d_state, st));
    if (measuring)
        if ((rc = filters_commit_keyframe(f, c, n_s, stepping.data(), kfm, st)) != HNET_OK) return rc;
    const AdvanceResult* h_res = o.h.res;
    for (int j = 0; j < n_a; j++) {
        const int i = order[j], id = ids[i];
        hnet_sessions::Sess& e = s->st[id];
        f->last_slot[id] = j;
        if (status[i] == HNET_ADV_WAIT_INIT) {
            if (!h_res[j].ok) {                                    // the frame is dropped: the session starts over (VioManager.cpp:158-162)
                f->t_seen[id] = e.t_push;
                e.count = 0;
                e.curr = 0;
                e.t = -1.0;
                continue;
            }
            status[i] = HNET_ADV_INITIALIZED;
            f->inited[id] = 1;
            f->t[id] = h_res[j].time0 > e.t_push ? h_res[j].time0 : e.t_push;
            e.count = 1;                                           // this frame is the session's first image; its ring slot stays the current one
            e.t = -1.0;
        } else {
            f->t[id] = e.t_push;
            if (j < n_s) {
                e.seq += (uint64_t)I;
                if (updates) updates[i] = o.h.upd[j];
                if (net_out)
                    for (int it = 0; it < I; it++) memcpy(net_out + ((size_t)it * n + i) * 72, o.h.net + ((size_t)it * B + j) * 72, 72 * sizeof(float));
            }
        }
        if (state_out) memcpy(state_out + i, o.h.work + j, sizeof(FilterRec));
    }
    return filters_accepted(f, n_s, hid, gate, refining > 0, measuring > 0, recovering > 0, t_begin, n_s ? I : 0);     // (the stepping sessions are the first n_s of the call's id table)
}

int hnet_filters_last_selection(hnet_filters* f, int id, hnet_imu* out, int cap, int* count) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = f->s->ctx;
    if (!f->cap) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_last_selection: feed not enabled");
    if (!count || id < 0 || id >= f->s->n || cap < 0 || (cap > 0 && !out)) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_last_selection: id / out / count");
    *count = 0;
    const int j = f->last_slot[id];
    if (j < 0) return HNET_OK;
    const AdvanceResult* h_res = filters_out_view(f, f->pin_out).res;
    const int m = h_res[j].ok ? h_res[j].n_sel : 0;
    if (m < 0 || m > f->cap + 2) return fail(c, HNET_ERR_DEVICE, "hnet_filters_last_selection: selection count out of range");
    *count = m;
    const int k = std::min(m, cap);
    if (k > 0) {
        HIPCHK(c, hipSetDevice(c->cfg.device_id));
        HIPCHK(c, hipMemcpyAsync(out, f->d_sel + (size_t)j * 2 * (f->cap + 2) + (f->cap + 2), (size_t)k * sizeof(hnet_imu), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return HNET_OK;
}

// ---- filters, innovation records (include/hnet.h): the records themselves come from filter_innovation_kernel inside hnet_filters_step / _advance ----

static_assert(sizeof(hnet_innovation) == sizeof(InnovRec), "hnet_innovation is the InnovRec layout");
static_assert((int)HNET_INNOV_NONE == (int)hnet_ekf::INNOV_NONE && (int)HNET_INNOV_USED == (int)hnet_ekf::INNOV_USED && (int)HNET_INNOV_REJECTED == (int)hnet_ekf::INNOV_REJECTED &&
              (int)HNET_INNOV_SINGULAR == (int)hnet_ekf::INNOV_SINGULAR && (int)HNET_INNOV_SKIPPED == (int)hnet_ekf::INNOV_SKIPPED, "HNET_INNOV_* are the header's flags");

// The output block with room for another kind of record: a new device block and pinned copy laid out for (innov, photo) and `extra_bytes` of zeroed device
// memory (*extra: the gates start open; the partials are scratch), the old blocks freed only when everything is there.  On failure the layout is the old
// one again and nothing of the object has changed.
static int filters_relayout(hnet_filters* f, bool innov, bool photo, bool refine, bool kfm, const char* who, void** extra, size_t extra_bytes) {
    hnet_ctx* c = f->s->ctx;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipStreamSynchronize(c->stream));                    // (nothing enqueued reads the old output block any more)
    const int B = c->cfg.max_batch;
    filters_out_layout(f, B, innov, photo, refine, kfm);
    uint8_t *d_out = nullptr, *pin_out = nullptr;
    void* d_extra = nullptr;
    hipError_t e = hipMalloc((void**)&d_out, f->out_bytes);
    if (e == hipSuccess) e = hipHostMalloc((void**)&pin_out, f->out_bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(&d_extra, extra_bytes);
    if (e == hipSuccess) e = hipMemsetAsync(d_extra, 0, extra_bytes, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        drop_dev(d_out); drop_pin(pin_out); drop_dev(d_extra);
        filters_out_layout(f, B, f->innov, f->photo, f->refine, f->kfm);
        return fail(c, HNET_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    }
    (void)hipFree(f->d_out);
    (void)hipHostFree(f->pin_out);
    f->d_out = d_out;
    f->pin_out = pin_out;
    *extra = d_extra;
    f->last_n = 0;                                                 // what last_priors / last_selection / last_innovations / last_photometric described went with the old block
    f->last_innov_n = 0;
    f->last_photo_n = 0;
    f->last_refine_n = 0;
    f->last_kfm_n = 0;
    f->last_kfmr_n = 0;
    std::fill(f->last_slot.begin(), f->last_slot.end(), -1);
    return HNET_OK;
}

int hnet_filters_enable_innovations(hnet_filters* f) {
    if (!f) return HNET_ERR_INVALID_ARG;
    if (f->innov) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_enable_innovations: already enabled");
    const int N = f->s->n;
    const int rc = filters_relayout(f, true, f->photo, f->refine, f->kfm, "hnet_filters_enable_innovations", (void**)&f->d_max_nis, (size_t)N * sizeof(double));
    if (rc != HNET_OK) return rc;
    f->innov_stats.assign(N, hnet_innovation_stats{0, 0, 0, 0.0, 0.0});
    f->innov = true;
    return HNET_OK;
}

int hnet_filters_set_nis_gate(hnet_filters* f, int id, double max_nis) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = f->s->ctx;
    if (!f->innov) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_set_nis_gate: innovations not enabled (hnet_filters_enable_innovations)");
    if (id < 0 || id >= f->s->n || !(max_nis >= 0.0)) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_set_nis_gate: id out of range, or max_nis negative or NaN");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipMemcpyAsync(f->d_max_nis + id, &max_nis, sizeof max_nis, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HNET_OK;
}

int hnet_filters_last_innovations(const hnet_filters* f, int n, hnet_innovation* out) {
    if (!f || !out) return HNET_ERR_INVALID_ARG;
    if (!f->innov || f->last_innov_n < 1) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_last_innovations: the last step ran without innovations");
    if (n != f->last_innov_n) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_last_innovations: n differs from the last step's");
    memcpy(out, filters_out_view(f, f->pin_out).innov, (size_t)f->iters * n * sizeof(InnovRec));
    return HNET_OK;
}

int hnet_filters_innovation_stats(const hnet_filters* f, int id, hnet_innovation_stats* out) {
    if (!f || !out) return HNET_ERR_INVALID_ARG;
    if (!f->innov || id < 0 || id >= f->s->n) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_innovation_stats: innovations not enabled or id out of range");
    *out = f->innov_stats[id];
    return HNET_OK;
}

int hnet_filters_reset_innovation_stats(hnet_filters* f, int id) {
    if (!f) return HNET_ERR_INVALID_ARG;
    if (!f->innov || id < 0 || id >= f->s->n) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_reset_innovation_stats: innovations not enabled or id out of range");
    f->innov_stats[id] = hnet_innovation_stats{0, 0, 0, 0.0, 0.0};
    return HNET_OK;
}

// ---- filters, photometric residual records (include/hnet.h): csrc/kernels_photo.hip on the step's pairs, inside hnet_filters_step / _advance ----

int hnet_filters_enable_photometric(hnet_filters* f) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = f->s->ctx;
    if (f->photo) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_enable_photometric: already enabled");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    // first the gates (none set) and the verdict words of the photometric gate: small, and made here so that hnet_filters_set_photo_gate only writes
    const int N = f->s->n, B = c->cfg.max_batch;
    hipError_t e = hipMalloc((void**)&f->d_photo_gate, (size_t)N * sizeof(PhotoGate));
    if (e == hipSuccess) e = hipMalloc((void**)&f->d_photo_verdict, (size_t)B * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemsetAsync(f->d_photo_gate, 0, (size_t)N * sizeof(PhotoGate), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(f->d_photo_verdict, 0, (size_t)B * sizeof(int32_t), c->stream);
    int rc = e == hipSuccess ? HNET_OK : fail(c, HNET_ERR_DEVICE, std::string("hnet_filters_enable_photometric: ") + hipGetErrorString(e));
    const size_t part = photo_partial_count(B, 2 + f->iters) * sizeof(PhotoRec);
    if (rc == HNET_OK) rc = filters_relayout(f, f->innov, true, false, f->kfm, "hnet_filters_enable_photometric", (void**)&f->d_photo_part, part);      // (synchronises)
    if (rc != HNET_OK) {
        drop_dev(f->d_photo_gate); drop_dev(f->d_photo_verdict);
        return rc;
    }
    f->photo_gate.assign(N, PhotoGate{0.0, 0, 0});
    f->photo_stats.assign(N, hnet_photo_stats{0, 0, 0, 0.0, 0.0});
    f->photo = true;
    return HNET_OK;
}

static_assert(sizeof(hnet_photo_residual) == sizeof(PhotoRec) && (int)HNET_PHOTO_DEGENERATE == PHOTO_DEGENERATE && (int)HNET_PHOTO_REJECTED == PHOTO_REJECTED,
              "hnet_photo_residual is the PhotoRec layout");

int hnet_filters_set_photo_gate(hnet_filters* f, int id, double max_ratio, int32_t min_inside) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = f->s->ctx;
    if (!f->photo) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_set_photo_gate: photometric records not enabled (hnet_filters_enable_photometric)");
    if (id < 0 || id >= f->s->n || !(max_ratio >= 0.0) || min_inside < 0 || min_inside > NPIX)
        return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_set_photo_gate: id out of range, max_ratio negative or NaN, or min_inside outside 0 .. 71680");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const PhotoGate g{max_ratio, min_inside, 0};
    HIPCHK(c, hipMemcpyAsync(f->d_photo_gate + id, &g, sizeof g, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    f->photo_gate[id] = g;
    return HNET_OK;
}

int hnet_filters_photo_stats(const hnet_filters* f, int id, hnet_photo_stats* out) {
    if (!f || !out) return HNET_ERR_INVALID_ARG;
    if (!f->photo || id < 0 || id >= f->s->n) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_photo_stats: photometric records not enabled or id out of range");
    *out = f->photo_stats[id];
    return HNET_OK;
}

int hnet_filters_reset_photo_stats(hnet_filters* f, int id) {
    if (!f) return HNET_ERR_INVALID_ARG;
    if (!f->photo || id < 0 || id >= f->s->n) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_reset_photo_stats: photometric records not enabled or id out of range");
    f->photo_stats[id] = hnet_photo_stats{0, 0, 0, 0.0, 0.0};
    return HNET_OK;
}

int hnet_filters_set_photo_gate_taps(hnet_filters* f, int from_global) {
    if (!f) return HNET_ERR_INVALID_ARG;
    f->photo_taps_global = from_global != 0;
    return HNET_OK;
}

int hnet_filters_last_photometric(const hnet_filters* f, int n, hnet_photo_residual* out) {
    if (!f || !out) return HNET_ERR_INVALID_ARG;
    if (!f->photo || f->last_photo_n < 1) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_last_photometric: the last step ran without photometric records");
    if (n != f->last_photo_n) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_last_photometric: n differs from the last step's");
    memcpy(out, filters_out_view(f, f->pin_out).photo, (size_t)n * (2 + f->iters) * sizeof(PhotoRec));
    return HNET_OK;
}

// ---- filters, the photometric fallback (include/hnet.h): csrc/kernels_filters_refine.hip around the robust alignment, inside hnet_filters_step / _advance ----

static_assert(sizeof(hnet_photo_refine) == sizeof(RefineRec) && offsetof(hnet_photo_refine, r_px) == offsetof(RefineRec, r_px) && offsetof(hnet_photo_refine, innov) == offsetof(RefineRec, r) &&
              offsetof(hnet_photo_refine, flags) == offsetof(RefineRec, flags) && sizeof(hnet_photo_refine_opts) == sizeof(RefineOpts) &&
              offsetof(hnet_photo_refine_opts, levels) == offsetof(RefineOpts, levels) && offsetof(hnet_photo_refine_opts, cov_scale) == offsetof(RefineOpts, cov_scale) &&
              offsetof(hnet_photo_refine_opts, max_mse) == offsetof(RefineOpts, max_mse), "hnet_photo_refine / _opts are the layouts of include/hnet_photo_refine.h");
static_assert((int)HNET_REFINE_ASKED == hnet_refine::ASKED && (int)HNET_REFINE_APPLIED == hnet_refine::APPLIED && (int)HNET_REFINE_NIS_REJECTED == hnet_refine::NIS_REJECTED &&
              (int)HNET_REFINE_S_SINGULAR == hnet_refine::S_SINGULAR && (int)HNET_REFINE_BAD_K_NET_COV == hnet_refine::BAD_K_NET_COV && (int)HNET_REFINE_STOPPED == hnet_refine::STOPPED &&
              (int)HNET_REFINE_NO_STEP == hnet_refine::NO_STEP && (int)HNET_REFINE_MSE_ABOVE_MAX == hnet_refine::MSE_ABOVE_MAX && (int)HNET_REFINE_NO_FACTOR == hnet_refine::NO_FACTOR &&
              (int)HNET_REFINE_NON_FINITE == hnet_refine::NON_FINITE && (int)HNET_REFINE_UNUSABLE == hnet_refine::UNUSABLE, "HNET_REFINE_* are the header's flags");

void hnet_photo_refine_default_opts(hnet_photo_refine_opts* o) {
    if (!o) return;
    RefineOpts d;
    hnet_refine::default_opts(d);
    memcpy(o, &d, sizeof d);
}

int hnet_filters_set_photo_refine(hnet_filters* f, int id, const hnet_photo_refine_opts* opts) {
    const char* who = "hnet_filters_set_photo_refine";
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = f->s->ctx;
    if (!f->photo) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": photometric records not enabled (hnet_filters_enable_photometric)");
    if (id < 0 || id >= f->s->n) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": id out of range");
    if (opts && f->kfm && f->kfm_on[id]) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": the session has the keyframe measurement on (hnet_filters_set_keyframe_measure)");
    hnet_photo_refine_opts o;
    memset(&o, 0, sizeof o);
    if (opts) {
        if (const int rc = photo_robust_check_opts(c, &opts->align, who); rc != HNET_OK) return rc;
        o = *opts;
        o.pad = o.align.pad = 0;                                   // (the sessions of a call are compared on the bytes of `align`)
        RefineOpts r;
        memcpy(&r, &o, sizeof r);
        if (!hnet_refine::opts_valid(r))
            return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": 1 <= levels <= 4, cov_scale > 0, sigma_floor_px >= 0, max_mse >= 0, all finite");
    }
    if (!opts && !f->refine) return HNET_OK;                       // (off, and never on)
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const int N = f->s->n, B = c->cfg.max_batch;
    if (!f->refine) {
        if (const int rc = ensure_pyr_scratch(c); rc != HNET_OK) return rc;
        RefineCfg* d_cfg = nullptr;
        HIPCHK(c, dalloc(&d_cfg, (size_t)N));
        hipError_t e = hipMemsetAsync(d_cfg, 0, (size_t)N * sizeof(RefineCfg), c->stream);
        int rc = e == hipSuccess ? HNET_OK : fail(c, HNET_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
        if (rc == HNET_OK) rc = filters_relayout(f, f->innov, f->photo, true, f->kfm, who, (void**)&f->d_refine_scratch, RefineScratch(nullptr, B, N).bytes);      // (synchronises)
        if (rc != HNET_OK) {
            drop_dev(d_cfg);
            return rc;
        }
        f->d_refine_cfg = d_cfg;
        f->refine_opts.assign(N, hnet_photo_refine_opts{});
        f->refine_on.assign(N, 0);
        f->refine_stats.assign(N, hnet_refine_stats{0, 0, 0, 0, 0.0, 0.0});
        f->refine = true;
    }
    const RefineCfg g{o.cov_scale, o.sigma_floor_px, o.max_mse, opts ? 1 : 0, 0};
    HIPCHK(c, hipMemcpyAsync(f->d_refine_cfg + id, &g, sizeof g, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    f->refine_opts[id] = o;
    f->refine_on[id] = opts ? 1 : 0;
    return HNET_OK;
}

int hnet_filters_last_refine(const hnet_filters* f, int n, hnet_photo_refine* out) {
    if (!f || !out) return HNET_ERR_INVALID_ARG;
    if (!f->refine || f->last_refine_n < 1) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_last_refine: the last step ran without a refining session");
    if (n != f->last_refine_n) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_last_refine: n differs from the last step's");
    memcpy(out, filters_out_view(f, f->pin_out).refine, (size_t)n * sizeof(RefineRec));
    return HNET_OK;
}

int hnet_filters_refine_stats(const hnet_filters* f, int id, hnet_refine_stats* out) {
    if (!f || !out) return HNET_ERR_INVALID_ARG;
    if (!f->refine || id < 0 || id >= f->s->n) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_refine_stats: refinement never turned on or id out of range");
    *out = f->refine_stats[id];
    return HNET_OK;
}

int hnet_filters_reset_refine_stats(hnet_filters* f, int id) {
    if (!f) return HNET_ERR_INVALID_ARG;
    if (!f->refine || id < 0 || id >= f->s->n) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_reset_refine_stats: refinement never turned on or id out of range");
    f->refine_stats[id] = hnet_refine_stats{0, 0, 0, 0, 0.0, 0.0};
    return HNET_OK;
}

// ---- filters, the keyframe track as an in-step measurement (include/hnet.h): csrc/kernels_filters_keyframe.hip around the keyframe track's
// launches (capi_keyframe.hip), inside hnet_filters_step / _advance ----

static_assert(sizeof(hnet_keyframe_measure) == sizeof(KfmRec) && offsetof(hnet_keyframe_measure, step_px) == offsetof(KfmRec, step_px) &&
              offsetof(hnet_keyframe_measure, z_px) == offsetof(KfmRec, z_px) && offsetof(hnet_keyframe_measure, r_px) == offsetof(KfmRec, r_px) &&
              offsetof(hnet_keyframe_measure, innov) == offsetof(KfmRec, r) && offsetof(hnet_keyframe_measure, flags) == offsetof(KfmRec, flags) &&
              sizeof(hnet_keyframe_measure_opts) == sizeof(KfmOpts) && offsetof(hnet_keyframe_measure_opts, cov_scale) == offsetof(KfmOpts, cov_scale) &&
              offsetof(hnet_keyframe_measure_opts, max_mse) == offsetof(KfmOpts, max_mse) && offsetof(hnet_keyframe_measure_opts, when) == offsetof(KfmOpts, when),
              "hnet_keyframe_measure / _opts are the layouts of include/hnet_keyframe_measure.h");
static_assert((int)HNET_KFM_ASKED == hnet_kfm::ASKED && (int)HNET_KFM_APPLIED == hnet_kfm::APPLIED && (int)HNET_KFM_NIS_REJECTED == hnet_kfm::NIS_REJECTED &&
              (int)HNET_KFM_S_SINGULAR == hnet_kfm::S_SINGULAR && (int)HNET_KFM_BAD_K_NET_COV == hnet_kfm::BAD_K_NET_COV && (int)HNET_KFM_STOPPED == hnet_kfm::STOPPED &&
              (int)HNET_KFM_NO_STEP == hnet_kfm::NO_STEP && (int)HNET_KFM_MSE_ABOVE_MAX == hnet_kfm::MSE_ABOVE_MAX && (int)HNET_KFM_NO_FACTOR == hnet_kfm::NO_FACTOR &&
              (int)HNET_KFM_NON_FINITE == hnet_kfm::NON_FINITE && (int)HNET_KFM_FIRST == hnet_kfm::FIRST && (int)HNET_KFM_TRACK_LOST == hnet_kfm::TRACK_LOST &&
              (int)HNET_KFM_TRACK_GAP == hnet_kfm::TRACK_GAP && (int)HNET_KFM_PREV_NOT_MEASURED == hnet_kfm::PREV_NOT_MEASURED &&
              (int)HNET_KFM_NO_INVERSE == hnet_kfm::NO_INVERSE && (int)HNET_KFM_NOT_SELECTED == hnet_kfm::NOT_SELECTED && (int)HNET_KFM_UNUSABLE == hnet_kfm::UNUSABLE &&
              (int)HNET_KFM_ALWAYS == hnet_kfm::ALWAYS && (int)HNET_KFM_IF_NONE == hnet_kfm::IF_NONE, "HNET_KFM_* are the header's values");

void hnet_keyframe_measure_default_opts(hnet_keyframe_measure_opts* o) {
    if (!o) return;
    KfmOpts d;
    hnet_kfm::default_opts(d);
    memcpy(o, &d, sizeof d);
}

int hnet_filters_set_keyframe_measure(hnet_filters* f, int id, const hnet_keyframe_measure_opts* opts) {
    const char* who = "hnet_filters_set_keyframe_measure";
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = f->s->ctx;
    if (!capi::keyframes_enabled(f->s)) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": keyframes are not enabled (hnet_sessions_enable_keyframes)");
    if (id < 0 || id >= f->s->n) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": id out of range");
    hnet_keyframe_measure_opts o;
    memset(&o, 0, sizeof o);
    if (opts) {
        if (f->refine && f->refine_on[id]) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": the session has refinement on (hnet_filters_set_photo_refine)");
        if (const int rc = photo_robust_check_opts(c, &opts->track.align, who); rc != HNET_OK) return rc;
        o = *opts;
        o.pad = o.track.pad = o.track.align.pad = 0;               // (the sessions of a call are compared on the bytes of `track`)
        KfmOpts r;
        memcpy(&r, &o, sizeof r);
        if (!hnet_kfm::opts_valid(r))
            return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": track: 1 <= levels <= 4, auto_rekey 0 / 1, max_age >= 0, 0 <= rekey_overlap <= 1, max_mse >= 0; "
                                                                    "cov_scale > 0, sigma_floor_px >= 0, max_mse >= 0, all finite; when ALWAYS or IF_NONE");
    }
    if (!opts && !f->kfm) return HNET_OK;                          // (off, and never on)
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const int N = f->s->n, B = c->cfg.max_batch;
    if (!f->kfm) {
        KfmCfg* d_cfg = nullptr;
        HIPCHK(c, dalloc(&d_cfg, (size_t)N));
        hipError_t e = hipMemsetAsync(d_cfg, 0, (size_t)N * sizeof(KfmCfg), c->stream);
        int rc = e == hipSuccess ? HNET_OK : fail(c, HNET_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
        if (rc == HNET_OK) rc = filters_relayout(f, f->innov, f->photo, f->refine, true, who, (void**)&f->d_kfm_scratch, KfmScratch(nullptr, B, N).bytes);      // (synchronises)
        if (rc != HNET_OK) {
            drop_dev(d_cfg);
            return rc;
        }
        f->d_kfm_cfg = d_cfg;
        f->kfm_opts.assign(N, hnet_keyframe_measure_opts{});
        f->kfm_on.assign(N, 0);
        f->kfm_stats.assign(N, hnet_keyframe_measure_stats{0, 0, 0, 0, 0.0, 0.0});
        f->kfm = true;
    }
    const KfmCfg g{o.cov_scale, o.sigma_floor_px, o.max_mse, o.when, opts ? 1 : 0};
    HIPCHK(c, hipMemcpyAsync(f->d_kfm_cfg + id, &g, sizeof g, hipMemcpyHostToDevice, c->stream));
    if (!opts) {                                                   // (a session that stops measuring has no previous in-step track when it starts again)
        const KfmScratch w(f->d_kfm_scratch, B, N);
        HIPCHK(c, hipMemsetAsync(w.prev_ok + id, 0, sizeof(int32_t), c->stream));
        if (f->kfmr) HIPCHK(c, hipMemsetAsync(KfmrScratch(f->d_kfmr_scratch, B, N).on + id, 0, sizeof(int32_t), c->stream));      // (and recovers no more)
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    f->kfm_opts[id] = o;
    f->kfm_on[id] = opts ? 1 : 0;
    if (!opts && f->kfmr) f->kfmr_on[id] = 0;
    return HNET_OK;
}

int hnet_filters_last_keyframe_measure(const hnet_filters* f, int n, hnet_keyframe_measure* out) {
    if (!f || !out) return HNET_ERR_INVALID_ARG;
    if (!f->kfm || f->last_kfm_n < 1) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_last_keyframe_measure: the last step ran without a measuring session");
    if (n != f->last_kfm_n) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_last_keyframe_measure: n differs from the last step's");
    memcpy(out, filters_out_view(f, f->pin_out).kfm, (size_t)n * sizeof(KfmRec));
    return HNET_OK;
}

// ---- filters, recovery inside the in-step track (include/hnet.h): csrc/kernels_filters_keyframe.hip around
// hnet_sessions_keyframe_track_recover's launches (capi_keyframe.hip) ----

static_assert(sizeof(hnet_keyframe_measure_recover) == sizeof(KfmrRec) && offsetof(hnet_keyframe_measure_recover, reloc) == offsetof(KfmrRec, reloc) &&
              sizeof(hnet_keyframe_relocalise_oriented) == sizeof(OrientedRelocRec) && sizeof(hnet_photo_search_hyp) == sizeof(SearchHyp) &&
              sizeof(hnet_keyframe_relocalise_opts) == sizeof(RelocOpts),
              "hnet_keyframe_measure_recover is the layout of include/hnet_keyframe_measure_recover.h; the table and the options are copied as they are");
static_assert((int)HNET_KFM_FROM_RELOC == hnet_kfmr::FROM_RELOC && (int)HNET_KFM_REATTACHED == hnet_kfmr::REATTACHED && (int)HNET_KFMR_UNUSABLE == hnet_kfmr::UNUSABLE,
              "HNET_KFM_FROM_RELOC / _REATTACHED and HNET_KFMR_UNUSABLE are the header's values");

int hnet_filters_set_keyframe_recover(hnet_filters* f, int id, const hnet_keyframe_relocalise_opts* reloc, const hnet_photo_search_hyp* hyps, int n_hyp) {
    const char* who = "hnet_filters_set_keyframe_recover";
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = f->s->ctx;
    if (id < 0 || id >= f->s->n) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": id out of range");
    if (!f->kfm || !f->kfm_on[id]) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": the session has no keyframe measurement on (hnet_filters_set_keyframe_measure)");
    const int N = f->s->n, B = c->cfg.max_batch;
    RelocOpts o;
    std::vector<SearchHyp> table(SEARCH_MAX_HYP);
    int n_table = 0;
    memset(&o, 0, sizeof o);
    memset(table.data(), 0, table.size() * sizeof(SearchHyp));
    if (reloc) {
        if (const int rc = capi::keyframes_recover_check(f->s, reloc, hyps, n_hyp, who, o, table.data(), &n_table); rc != HNET_OK) return rc;
    } else if (!f->kfmr) {
        return HNET_OK;                                            // (off, and never on)
    }
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    if (reloc)
        if (const int rc = capi::keyframes_instep_recover_ensure(f->s, who); rc != HNET_OK) return rc;
    if (!f->kfmr) {
        f->kfmr = true;                                            // (filters_out_layout reads it)
        const int rc = filters_relayout(f, f->innov, f->photo, f->refine, f->kfm, who, (void**)&f->d_kfmr_scratch, KfmrScratch(nullptr, B, N).bytes);      // (synchronises)
        if (rc != HNET_OK) {
            f->kfmr = false;
            filters_out_layout(f, B, f->innov, f->photo, f->refine, f->kfm);
            return rc;
        }
        f->kfmr_opts.assign(N, RelocOpts{});
        f->kfmr_tab.assign((size_t)N * SEARCH_MAX_HYP, SearchHyp{});
        f->kfmr_n_hyp.assign(N, 0);
        f->kfmr_on.assign(N, 0);
    }
    const KfmrScratch w(f->d_kfmr_scratch, B, N);
    const int32_t on = reloc ? 1 : 0;
    HIPCHK(c, hipMemcpyAsync(w.hyps + (size_t)id * SEARCH_MAX_HYP, table.data(), (size_t)SEARCH_MAX_HYP * sizeof(SearchHyp), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(w.on + id, &on, sizeof on, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    f->kfmr_opts[id] = o;
    memcpy(&f->kfmr_tab[(size_t)id * SEARCH_MAX_HYP], table.data(), (size_t)SEARCH_MAX_HYP * sizeof(SearchHyp));
    f->kfmr_n_hyp[id] = n_table;
    f->kfmr_on[id] = (uint8_t)on;
    return HNET_OK;
}

int hnet_filters_last_keyframe_recover(const hnet_filters* f, int n, hnet_keyframe_measure_recover* out) {
    if (!f || !out) return HNET_ERR_INVALID_ARG;
    if (!f->kfmr || f->last_kfmr_n < 1) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_last_keyframe_recover: the last step ran without a recovering session");
    if (n != f->last_kfmr_n) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_last_keyframe_recover: n differs from the last step's");
    const OutView h = filters_out_view(f, f->pin_out);
    for (int j = 0; j < n; j++) {
        memcpy(&out[j].m, h.kfm + j, sizeof(KfmRec));
        memcpy(&out[j].reloc, h.kfmr + j, sizeof(OrientedRelocRec));
    }
    return HNET_OK;
}

int hnet_filters_keyframe_measure_stats(const hnet_filters* f, int id, hnet_keyframe_measure_stats* out) {
    if (!f || !out) return HNET_ERR_INVALID_ARG;
    if (!f->kfm || id < 0 || id >= f->s->n) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_keyframe_measure_stats: the keyframe measurement never turned on or id out of range");
    *out = f->kfm_stats[id];
    return HNET_OK;
}

int hnet_filters_reset_keyframe_measure_stats(hnet_filters* f, int id) {
    if (!f) return HNET_ERR_INVALID_ARG;
    if (!f->kfm || id < 0 || id >= f->s->n)
        return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_reset_keyframe_measure_stats: the keyframe measurement never turned on or id out of range");
    f->kfm_stats[id] = hnet_keyframe_measure_stats{0, 0, 0, 0, 0.0, 0.0};
    return HNET_OK;
}

// ---- filters, between frames (include/hnet.h): hnet_filters_predict.  Read-only: nothing of the filters' or the sessions' bookkeeping is written.

static_assert(sizeof(hnet_odometry) == sizeof(PredictOut), "hnet_odometry is the PredictOut layout");
static_assert(HNET_PRED_OK == PRED_OK && HNET_PRED_NO_STATE == PRED_NO_STATE && HNET_PRED_WAIT_IMU == PRED_WAIT_IMU && HNET_PRED_AT_STATE == PRED_AT_STATE,
              "HNET_PRED_* are the kernel's codes");

// the call's buffers, made once: the kernel's scratch is its own, so that hnet_filters_last_selection keeps describing the last advance
static int predict_buffers(hnet_filters* f) {
    if (f->d_pred) return HNET_OK;
    hnet_ctx* c = f->s->ctx;
    const int B = c->cfg.max_batch;
    f->off_pred_out = al256((size_t)B * sizeof(PredictJob));
    const size_t bytes = f->off_pred_out + (size_t)B * sizeof(PredictOut);
    hipError_t e = hipMalloc((void**)&f->d_pred_sel, (size_t)B * 2 * (f->cap + 2) * sizeof(hnet_ekf::ImuData));
    if (e == hipSuccess) e = hipHostMalloc((void**)&f->pin_pred, bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreate(&f->pred_time.ev0);
    if (e == hipSuccess) e = hipEventCreate(&f->pred_time.ev1);
    if (e == hipSuccess) e = hipMalloc((void**)&f->d_pred, bytes);
    if (e != hipSuccess) {
        filters_drop_predict(f);
        return fail(c, HNET_ERR_DEVICE, std::string("hnet_filters_predict: ") + hipGetErrorString(e));
    }
    return HNET_OK;
}

// What hnet_filters_predict and hnet_filters_predict_cov (`who`, for the messages) do before they enqueue anything: the argument checks in their order
// (`missing`: null, or the names of the caller's own pointers of which one is null), the device, the caller's buffers (`buffers`: made by its first call)
// and the job of every listed session in `*job`, the caller's pinned job table, which exists once `buffers` has run.
static int predict_prepare(hnet_filters* f, const char* who, const char* missing, int n, const int32_t* ids, const double* t_query, int (*buffers)(hnet_filters*),
                           uint8_t* const* job) {
    hnet_ctx* c = f->s->ctx;
    if (!f->cap) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": feed not enabled (hnet_filters_enable_feed)");
    if (missing) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": " + missing);
    int rc = sessions_check_ids(f->s, n, ids);
    if (rc != HNET_OK) return rc;
    for (int i = 0; i < n; i++)
        if (!std::isfinite(t_query[i])) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": t_query must be finite");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    if ((rc = buffers(f)) != HNET_OK) return rc;
    PredictJob* jb = reinterpret_cast<PredictJob*>(*job);
    for (int i = 0; i < n; i++) {
        const int id = ids[i];
        const double dt = f->cam_imu_dt[id];
        int st = PRED_OK;                                          // (the kernel reports AT_STATE from the device's own state time)
        if (!f->inited[id]) st = PRED_NO_STATE;
        else if (t_query[i] > f->t[id] && !(t_query[i] < f->imu_newest[id] - dt)) st = PRED_WAIT_IMU;
        jb[i] = PredictJob{t_query[i], dt, id, st};
    }
    return HNET_OK;
}
// the two events of a timed launch, each recorded where the caller stands in the stream, and the time between them once the stream has been drained
static hipError_t timed_record(const TimedLaunch& t, hipEvent_t ev, hipStream_t st) { return t.timed ? hipEventRecord(ev, st) : hipSuccess; }
static hipError_t timed_read(TimedLaunch& t) {
    float ms = 0;
    const hipError_t e = t.timed ? hipEventElapsedTime(&ms, t.ev0, t.ev1) : hipSuccess;
    if (t.timed && e == hipSuccess) t.ms = ms;
    return e;
}

int hnet_filters_predict(hnet_filters* f, int n, const int32_t* ids, const double* t_query, hnet_odometry* out) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_sessions* s = f->s;
    hnet_ctx* c = s->ctx;
    const int rc = predict_prepare(f, "hnet_filters_predict", !t_query || !out ? "t_query / out" : nullptr, n, ids, t_query, predict_buffers, &f->pin_pred);
    if (rc != HNET_OK) return rc;
    hipStream_t st = c->stream;
    PredictOut* d_out = reinterpret_cast<PredictOut*>(f->d_pred + f->off_pred_out);
    HIPCHK(c, hipMemcpyAsync(f->d_pred, f->pin_pred, (size_t)n * sizeof(PredictJob), hipMemcpyHostToDevice, st));
    HIPCHK(c, timed_record(f->pred_time, f->pred_time.ev0, st));
    HIPCHK(c, launch_filter_predict(reinterpret_cast<const PredictJob*>(f->d_pred), n, s->n, f->cap, f->d_ring, f->d_meta, f->d_state, f->d_params, f->d_pred_sel,
                                    d_out, st));
    HIPCHK(c, timed_record(f->pred_time, f->pred_time.ev1, st));
    HIPCHK(c, hipMemcpyAsync(f->pin_pred + f->off_pred_out, d_out, (size_t)n * sizeof(PredictOut), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    memcpy(out, f->pin_pred + f->off_pred_out, (size_t)n * sizeof(PredictOut));
    HIPCHK(c, timed_read(f->pred_time));
    return HNET_OK;
}

// ---- hnet_filters_predict_cov: the predict's record with the covariance at the query time.  Read-only in the same sense.

static_assert(sizeof(hnet_odometry_cov) == sizeof(PredictCovOut), "hnet_odometry_cov is the PredictCovOut layout");

// the call's own job / output block, made once for max_batch sessions with the full covariances; the scratch is the predict's (predict_buffers first)
static int predict_cov_buffers(hnet_filters* f) {
    if (const int rc = predict_buffers(f); rc != HNET_OK) return rc;
    if (f->d_pcov) return HNET_OK;
    hnet_ctx* c = f->s->ctx;
    const int B = c->cfg.max_batch;
    f->off_pcov_out = al256((size_t)B * sizeof(PredictJob));
    const size_t bytes = f->off_pcov_out + (size_t)B * (sizeof(PredictOut) + sizeof(PredictCovOut) + (size_t)hnet_ekf::NS * hnet_ekf::NS * sizeof(double));
    hipError_t e = hipHostMalloc((void**)&f->pin_pcov, bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreate(&f->pcov_time.ev0);
    if (e == hipSuccess) e = hipEventCreate(&f->pcov_time.ev1);
    if (e == hipSuccess) e = hipMalloc((void**)&f->d_pcov, bytes);
    if (e != hipSuccess) {
        filters_drop_predict_cov(f);
        return fail(c, HNET_ERR_DEVICE, std::string("hnet_filters_predict_cov: ") + hipGetErrorString(e));
    }
    return HNET_OK;
}

int hnet_filters_predict_cov(hnet_filters* f, int n, const int32_t* ids, const double* t_query, hnet_odometry* out, hnet_odometry_cov* cov_out, double* full_cov) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_sessions* s = f->s;
    hnet_ctx* c = s->ctx;
    const int rc = predict_prepare(f, "hnet_filters_predict_cov", !t_query || !out || !cov_out ? "t_query / out / cov_out" : nullptr, n, ids, t_query,
                                   predict_cov_buffers, &f->pin_pcov);
    if (rc != HNET_OK) return rc;
    hipStream_t st = c->stream;
    const size_t off_cov = f->off_pcov_out + (size_t)n * sizeof(PredictOut), off_full = off_cov + (size_t)n * sizeof(PredictCovOut);
    const size_t full_bytes = full_cov ? (size_t)n * hnet_ekf::NS * hnet_ekf::NS * sizeof(double) : 0;
    HIPCHK(c, hipMemcpyAsync(f->d_pcov, f->pin_pcov, (size_t)n * sizeof(PredictJob), hipMemcpyHostToDevice, st));
    HIPCHK(c, timed_record(f->pcov_time, f->pcov_time.ev0, st));
    HIPCHK(c, launch_filter_predict_cov(reinterpret_cast<const PredictJob*>(f->d_pcov), n, s->n, f->cap, f->d_ring, f->d_meta, f->d_state, f->d_params, f->d_pred_sel,
                                        reinterpret_cast<PredictOut*>(f->d_pcov + f->off_pcov_out), reinterpret_cast<PredictCovOut*>(f->d_pcov + off_cov),
                                        full_cov ? reinterpret_cast<double*>(f->d_pcov + off_full) : nullptr, st));
    HIPCHK(c, timed_record(f->pcov_time, f->pcov_time.ev1, st));
    HIPCHK(c, hipMemcpyAsync(f->pin_pcov + f->off_pcov_out, f->d_pcov + f->off_pcov_out, off_full + full_bytes - f->off_pcov_out, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    memcpy(out, f->pin_pcov + f->off_pcov_out, (size_t)n * sizeof(PredictOut));
    memcpy(cov_out, f->pin_pcov + off_cov, (size_t)n * sizeof(PredictCovOut));
    if (full_cov) memcpy(full_cov, f->pin_pcov + off_full, full_bytes);
    HIPCHK(c, timed_read(f->pcov_time));
    return HNET_OK;
}

double hnet_filters_last_predict_cov_device_ms(hnet_filters* f) {
    if (!f) return NAN;
    f->pcov_time.timed = true;
    return f->pcov_time.ms;
}

double hnet_filters_newest_imu_time(const hnet_filters* f, int id) {
    if (!f || !f->cap || id < 0 || id >= f->s->n || !std::isfinite(f->imu_newest[id])) return NAN;
    return f->imu_newest[id];
}

double hnet_filters_last_predict_device_ms(hnet_filters* f) {
    if (!f) return NAN;
    f->pred_time.timed = true;
    return f->pred_time.ms;
}

}  // extern "C"
