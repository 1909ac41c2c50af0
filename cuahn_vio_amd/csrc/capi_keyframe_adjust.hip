// capi_keyframe_adjust.hip — hnet_keyframe_adjust_default_opts, hnet_op_keyframe_adjust_solve, hnet_op_keyframe_adjust,
// hnet_sessions_enable_keyframe_adjust and hnet_sessions_keyframe_adjust of include/hnet.h (keyframe_adjust_dev.h, csrc/kernels_keyframe_adjust.hip;
// DESIGN 7ad): a keyframe map adjusted jointly.  The operator-level calls own their buffers as device temporaries.  The sessions call reads the map, the
// states, the staging arrays and the alignment scratch of the keyframe store (keyframes_internal.h) and owns its tables, records and pinned blocks,
// allocated by its enable: additive, a store whose adjustment was never enabled holds a null pointer and allocates and
// launches nothing here.  The jobs of a call run in ROUNDS of max_batch alignments, because the alignment's scratch is sized by max_batch; the host
// needs the job counts to size the rounds, so a call has TWO synchronisations: one after the pairs kernel, one at the end.
#include "keyframes_internal.h"

#include <memory>

using namespace hnet;
using namespace capi;

namespace ka = hnet_adjust;

static_assert(sizeof(hnet_keyframe_adjust) == sizeof(AdjustRec) && offsetof(hnet_keyframe_adjust, n_pairs) == offsetof(AdjustRec, n_pairs) &&
              offsetof(hnet_keyframe_adjust, adjusted_mask) == offsetof(AdjustRec, adjusted_mask) && offsetof(hnet_keyframe_adjust, cost0) == offsetof(AdjustRec, cost0) &&
              offsetof(hnet_keyframe_adjust, delta_px) == offsetof(AdjustRec, delta_px) && offsetof(hnet_keyframe_adjust, h_origin_key) == offsetof(AdjustRec, h_origin_key) &&
              offsetof(hnet_keyframe_adjust, edge) == offsetof(AdjustRec, edge) && sizeof(hnet_keyframe_adjust_edge) == sizeof(AdjustEdge) &&
              offsetof(hnet_keyframe_adjust_edge, offsets_px) == offsetof(AdjustEdge, offsets_px) && offsetof(hnet_keyframe_adjust_edge, r0_px) == offsetof(AdjustEdge, r0_px) &&
              sizeof(hnet_keyframe_adjust_opts) == sizeof(AdjustOpts) && offsetof(hnet_keyframe_adjust_opts, min_grid) == offsetof(AdjustOpts, min_grid) &&
              offsetof(hnet_keyframe_adjust_opts, weighting) == offsetof(AdjustOpts, weighting) && offsetof(hnet_keyframe_adjust_opts, mse_floor) == offsetof(AdjustOpts, mse_floor) &&
              offsetof(hnet_keyframe_adjust_opts, max_shift_px) == offsetof(AdjustOpts, max_shift_px) && offsetof(hnet_keyframe_adjust_opts, apply) == offsetof(AdjustOpts, apply),
              "hnet_keyframe_adjust / _edge / _opts are the layouts of include/hnet_keyframe_adjust.h");
static_assert((int)HNET_ADJ_FEW_ENTRIES == ka::ADJ_FEW_ENTRIES && (int)HNET_ADJ_NO_EDGES == ka::ADJ_NO_EDGES && (int)HNET_ADJ_SINGULAR == ka::ADJ_SINGULAR &&
              (int)HNET_ADJ_NO_GAIN == ka::ADJ_NO_GAIN && (int)HNET_ADJ_SHIFT_ABOVE_MAX == ka::ADJ_SHIFT_ABOVE_MAX && (int)HNET_ADJ_CHAIN == ka::ADJ_CHAIN &&
              (int)HNET_ADJ_ADJUSTED == ka::ADJ_ADJUSTED && (int)HNET_ADJ_CONVERGED == ka::ADJ_CONVERGED && (int)HNET_ADJ_EDGE_ACCEPTED == ka::EDGE_ACCEPTED &&
              (int)HNET_ADJ_EDGE_STOPPED == ka::EDGE_STOPPED && (int)HNET_ADJ_EDGE_MSE_ABOVE_MAX == ka::EDGE_MSE_ABOVE_MAX &&
              (int)HNET_ADJ_EDGE_NON_FINITE == ka::EDGE_NON_FINITE && (int)HNET_ADJ_EDGE_LOW_OVERLAP == ka::EDGE_LOW_OVERLAP &&
              (int)HNET_ADJ_EDGE_CLOSURE_ABOVE_MAX == ka::EDGE_CLOSURE_ABOVE_MAX && (int)HNET_ADJ_EDGE_NO_RELATIVE == ka::EDGE_NO_RELATIVE &&
              (int)HNET_ADJ_WEIGHT_UNIT == ka::WEIGHT_UNIT && (int)HNET_ADJ_WEIGHT_INFO == ka::WEIGHT_INFO && HNET_ADJ_MAX_EDGES == ka::MAX_PAIRS &&
              HNET_ADJ_MAX_TRIALS == ka::MAX_TRIALS, "HNET_ADJ_* are the header's");

namespace {

// the adjustment of a store: sized at its enable for max_batch B
struct KeyAdjust : KeyLayer {
    int32_t* d_ids = nullptr;                  // device [B]
    AdjustJobs* tab = nullptr;                 // device [B]
    double* infos = nullptr;                   // device [B][28][64]
    uint8_t* d_out = nullptr;                  // device: a call's results {records [n] | level-0 records [n][28]}, packed for ONE download
    int32_t* pin_in = nullptr;                 // pinned: the ids,
    AdjustJobs* pin_tab = nullptr;             // the job tables,
    uint8_t* pin_out = nullptr;                // the results
};

constexpr size_t INFO_DOUBLES = (size_t)ADJUST_MAX_PAIRS * ADJUST_INFO, EDGE_RECS_BYTES = (size_t)ADJUST_MAX_PAIRS * sizeof(RobustRec);
size_t out_bytes(int n, bool edge_recs) { return (size_t)n * (sizeof(AdjustRec) + (edge_recs ? EDGE_RECS_BYTES : 0)); }

// o <- *opts with its pads zeroed, or the context's error
int check_opts(hnet_ctx* c, const hnet_keyframe_adjust_opts* opts, const char* who, AdjustOpts& o) {
    if (!opts) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": opts");
    const int rc = photo_robust_check_opts(c, &opts->align, who);
    if (rc != HNET_OK) return rc;
    memcpy(&o, opts, sizeof o);
    o.pad = 0;
    o.align.pad = 0;
    if (!ka::opts_valid(o))
        return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": opts: 1 <= levels <= 4, 1 <= min_grid <= 64, 0 <= min_overlap <= 1, max_mse, max_closure_px and "
                                                                "max_shift_px >= 0, weighting 0 / 1, 1 <= max_trials <= 64, mse_floor > 0, 0 < lambda0 <= 1e100, eps_px >= 0, "
                                                                "apply 0 / 1, all finite");
    return HNET_OK;
}

// what one adjustment runs on: the source, the call's device ids, its tables and records, the staging pair and the alignment's scratch for B pairs
struct AdjustRun {
    AdjustSource src; const int32_t* d_ids; int n; AdjustJobs* tab; AdjustRec* rec; double* infos; RobustRec* edge_recs; AlignScratch al; uint8_t *prev, *curr;
    AdjustJobs* h_tab;                         // host [n]: where the job tables are downloaded to
};

// The launches of one call on the stream, behind its upload: the pairs, the FIRST synchronisation (the job tables size the rounds), per round of at most
// max_batch jobs {gather, the unchanged robust alignment, edges}, and the solve.  The caller downloads the records and synchronises again.
int enqueue_adjust(hnet_ctx* c, const AdjustRun& r, const AdjustOpts& o) {
    const int B = c->cfg.max_batch;
    const size_t pyr = (size_t)B * PYR_BYTES;
    hipStream_t st = c->stream;
    HIPCHK(c, launch_keyframe_adjust_pairs(r.d_ids, r.n, r.src, o.min_grid, r.tab, r.rec, st));
    HIPCHK(c, hipMemcpyAsync(r.h_tab, r.tab, (size_t)r.n * sizeof(AdjustJobs), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    int total = 0;
    for (int b = 0; b < r.n; b++) total += std::min(std::max(r.h_tab[b].count, 0), ADJUST_MAX_PAIRS);
    if (r.edge_recs) HIPCHK(c, hipMemsetAsync(r.edge_recs, 0, (size_t)r.n * EDGE_RECS_BYTES, st));
    for (int first = 0; first < total; first += B) {
        const int nq = std::min(B, total - first);
        HIPCHK(c, launch_keyframe_adjust_gather(r.d_ids, r.n, r.src, r.tab, first, nq, r.prev, r.curr, r.al.x0, st));
        HIPCHK(c, launch_photo_align_robust(r.prev, r.curr, nq, r.al.x0, o.align, o.levels, c->pyr_scratch, c->pyr_scratch + pyr, r.al.start, r.al.part, r.al.work,
                                            r.al.rec, st));
        HIPCHK(c, launch_keyframe_adjust_edge(r.n, r.tab, first, nq, r.al.rec, o, r.rec, r.infos, r.edge_recs, st));
    }
    HIPCHK(c, launch_keyframe_adjust_solve(r.d_ids, r.n, r.src, r.infos, o, r.rec, st));
    return HNET_OK;
}

}  // namespace

extern "C" {

void hnet_keyframe_adjust_default_opts(hnet_keyframe_adjust_opts* o) {
    if (!o) return;
    AdjustOpts d;
    ka::default_opts(d);
    memcpy(o, &d, sizeof d);
}

// ONE upload {id 0 | entries [m] | the seeded record | infos}, the solve, ONE download of the record, one synchronisation
int hnet_op_keyframe_adjust_solve(hnet_ctx* c, int m, const hnet_keyframe_map_entry* entries, int n_edges, const hnet_keyframe_adjust_edge* edges,
                                  const double* edge_infos, const hnet_keyframe_adjust_opts* opts, hnet_keyframe_adjust* out) {
    const char* who = "hnet_op_keyframe_adjust_solve";
    if (!c) return HNET_ERR_INVALID_ARG;
    if (!entries || !out || (n_edges > 0 && !edges)) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": entries / edges / out");
    if (m < 1 || m > ka::MAX_ENTRIES || n_edges < 0 || n_edges > ka::MAX_PAIRS) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": 1 <= m <= 8, 0 <= n_edges <= 28");
    AdjustOpts o;
    const int rc = check_opts(c, opts, who, o);
    if (rc != HNET_OK) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const KeyUpload up(m, KeyUpload::SEED | (edge_infos ? KeyUpload::INFOS : 0));      // (the record with its rows, the information matrices)
    std::vector<uint8_t> h_in(up.total, 0);
    memcpy(h_in.data() + up.entry, entries, (size_t)m * sizeof(MapEntry));
    AdjustRec* seed = reinterpret_cast<AdjustRec*>(h_in.data() + up.seed);
    seed->n_jobs = n_edges;
    if (n_edges) memcpy(seed->edge, edges, (size_t)n_edges * sizeof(AdjustEdge));
    if (edge_infos) memcpy(h_in.data() + up.infos, edge_infos, (size_t)n_edges * ADJUST_INFO * sizeof(double));
    DevTemps t;
    uint8_t* d_in = nullptr;
    HIPCHK(c, t.alloc(&d_in, up.total));
    const AdjustSource src{nullptr, reinterpret_cast<MapEntry*>(d_in + up.entry), nullptr, nullptr, 1, m};
    AdjustRec* d_rec = reinterpret_cast<AdjustRec*>(d_in + up.seed);
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(d_in, h_in.data(), up.total, hipMemcpyHostToDevice, st));
    HIPCHK(c, launch_keyframe_adjust_solve(reinterpret_cast<const int32_t*>(d_in), 1, src, edge_infos ? reinterpret_cast<const double*>(d_in + up.infos) : nullptr, o,
                                           d_rec, st));
    AdjustRec h_rec;
    HIPCHK(c, hipMemcpyAsync(&h_rec, d_rec, sizeof h_rec, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    memcpy(out, &h_rec, sizeof h_rec);
    return HNET_OK;
}

// ONE upload {id 0 | entries [m] | images [m]}, the launches of enqueue_adjust with their synchronisation, ONE download {record | level-0 records}, the
// second synchronisation
int hnet_op_keyframe_adjust(hnet_ctx* c, int m, const uint8_t* images, const hnet_keyframe_map_entry* entries, const hnet_keyframe_adjust_opts* opts,
                            hnet_keyframe_adjust* out, hnet_photo_robust* out_edge_records) {
    const char* who = "hnet_op_keyframe_adjust";
    if (!c) return HNET_ERR_INVALID_ARG;
    if (!images || !entries || !out) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": images / entries / out");
    if (m < 1 || m > ka::MAX_ENTRIES) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": 1 <= m <= 8");
    AdjustOpts o;
    const int rc = check_opts(c, opts, who, o);
    if (rc != HNET_OK) return rc;
    o.apply = 0;                                                           // (there is no map to write: the record holds the matrices)
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const int B = c->cfg.max_batch;
    if (const int e = ensure_pyr_scratch(c); e != HNET_OK) return e;
    const KeyUpload up(m, KeyUpload::IMAGES);
    const size_t out_total = out_bytes(1, out_edge_records != nullptr);
    std::vector<uint8_t> h_in(up.total, 0), h_out(out_total);
    memcpy(h_in.data() + up.entry, entries, (size_t)m * sizeof(MapEntry));
    memcpy(h_in.data() + up.images, images, (size_t)m * NPIX);
    DevTemps t;
    uint8_t *d_in = nullptr, *d_out = nullptr, *d_stage = nullptr;
    AdjustRun r{};
    HIPCHK(c, t.alloc(&d_in, up.total));
    HIPCHK(c, t.alloc(&d_out, out_total));
    HIPCHK(c, t.alloc(&d_stage, 2 * (size_t)B * NPIX));
    HIPCHK(c, t.alloc(&r.tab, 1));
    HIPCHK(c, t.alloc(&r.infos, INFO_DOUBLES));
    HIPCHK(c, t.alloc(&r.al.rec, (size_t)HNET_ALIGN_MAX_LEVELS * B));
    HIPCHK(c, t.alloc(&r.al.start, (size_t)B));
    HIPCHK(c, t.alloc(&r.al.work, (size_t)B));
    HIPCHK(c, t.alloc(&r.al.part, (size_t)B * PHOTO_SLICES));
    HIPCHK(c, t.alloc(&r.al.x0, (size_t)B * 8));
    AdjustJobs h_tab;
    r.src = AdjustSource{d_in + up.images, reinterpret_cast<MapEntry*>(d_in + up.entry), nullptr, nullptr, 1, m};
    r.d_ids = reinterpret_cast<const int32_t*>(d_in);
    r.n = 1;
    r.rec = reinterpret_cast<AdjustRec*>(d_out);
    r.edge_recs = out_edge_records ? reinterpret_cast<RobustRec*>(d_out + sizeof(AdjustRec)) : nullptr;
    r.prev = d_stage;
    r.curr = d_stage + (size_t)B * NPIX;
    r.h_tab = &h_tab;
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(d_in, h_in.data(), up.total, hipMemcpyHostToDevice, st));
    if (const int e = enqueue_adjust(c, r, o); e != HNET_OK) return e;
    HIPCHK(c, hipMemcpyAsync(h_out.data(), d_out, out_total, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    memcpy(out, h_out.data(), sizeof(AdjustRec));
    if (out_edge_records) memcpy(out_edge_records, h_out.data() + sizeof(AdjustRec), EDGE_RECS_BYTES);
    return HNET_OK;
}

int hnet_sessions_enable_keyframe_adjust(hnet_sessions* s) {
    const char* who = "hnet_sessions_enable_keyframe_adjust";
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    hnet_keyframes* k = s->kf;
    if (!k || !k->map) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": the keyframe map is not enabled (hnet_sessions_enable_keyframe_map)");
    if (k->adjust) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": the keyframe adjustment is already enabled");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const size_t B = (size_t)c->cfg.max_batch;
    auto a = std::make_unique<KeyAdjust>();
    hipError_t e = a->mem.alloc(&a->d_ids, B);
    if (e == hipSuccess) e = a->mem.alloc(&a->tab, B);
    if (e == hipSuccess) e = a->mem.alloc(&a->infos, B * INFO_DOUBLES);
    if (e == hipSuccess) e = a->mem.alloc(&a->d_out, out_bytes((int)B, true));
    if (e == hipSuccess) e = a->mem.alloc_pinned(&a->pin_in, B);
    if (e == hipSuccess) e = a->mem.alloc_pinned(&a->pin_tab, B);
    if (e == hipSuccess) e = a->mem.alloc_pinned(&a->pin_out, out_bytes((int)B, true));
    if (e != hipSuccess) return fail(c, HNET_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    k->adjust = a.release();
    return HNET_OK;
}

// ONE upload {ids}, the launches of enqueue_adjust inside the store's events with their synchronisation, ONE download {records | level-0
// records}, the second synchronisation
int hnet_sessions_keyframe_adjust(hnet_sessions* s, int n, const int32_t* ids, const hnet_keyframe_adjust_opts* opts, hnet_keyframe_adjust* out,
                                  hnet_photo_robust* out_edge_records) {
    const char* who = "hnet_sessions_keyframe_adjust";
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    hnet_keyframes* k = s->kf;
    if (!k || !k->map || !k->adjust)
        return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": the keyframe adjustment is not enabled (hnet_sessions_enable_keyframe_adjust)");
    KeyAdjust* a = static_cast<KeyAdjust*>(k->adjust);
    if (!out) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": out");
    AdjustOpts o;
    int rc = check_opts(c, opts, who, o);
    if (rc != HNET_OK) return rc;
    if ((rc = sessions_check_ids(s, n, ids)) != HNET_OK) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    for (int i = 0; i < n; i++) a->pin_in[i] = ids[i];
    const size_t recs = (size_t)n * sizeof(AdjustRec), total = out_bytes(n, out_edge_records != nullptr);
    AdjustRun r{};
    r.src = adjust_source(k);
    r.d_ids = a->d_ids;
    r.n = n;
    r.tab = a->tab;
    r.rec = reinterpret_cast<AdjustRec*>(a->d_out);
    r.infos = a->infos;
    r.edge_recs = out_edge_records ? reinterpret_cast<RobustRec*>(a->d_out + recs) : nullptr;
    r.al = KeyScratch(k->scratch, c->cfg.max_batch).align();
    r.prev = (uint8_t*)c->stage_prev;
    r.curr = (uint8_t*)c->stage_curr;
    r.h_tab = a->pin_tab;
    if ((rc = begin_call(c, k, a->d_ids, a->pin_in, (size_t)n * sizeof(int32_t))) != HNET_OK) return rc;
    if ((rc = enqueue_adjust(c, r, o)) != HNET_OK) return rc;
    if ((rc = finish_call(c, k, a->d_out, a->pin_out, nullptr, total)) != HNET_OK) return rc;
    memcpy(out, a->pin_out, recs);
    if (out_edge_records) memcpy(out_edge_records, a->pin_out + recs, (size_t)n * EDGE_RECS_BYTES);
    return HNET_OK;
}

}  // extern "C"
