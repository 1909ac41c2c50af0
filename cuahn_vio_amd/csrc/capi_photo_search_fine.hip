// capi_photo_search_fine.hip — hnet_photo_search_fine_default_opts / _yaw_table, hnet_op_photo_search_fine and hnet_sessions_photo_search_fine of
// include/hnet.h (photo_search_fine_dev.h, csrc/kernels_photo_search_fine.hip): the oriented coarse search followed by the fine stage around
// its winner on level-2 thumbnails.  Both calls own their thumbnails, tables, records and score tables as device temporaries: nothing of the context's
// pyramid scratch, events or timings is touched.  The relocalisation that runs the same kernels on a session's picked candidate is capi_keyframe.hip's.
#include "sessions_internal.h"
#include "photo_search_fine_dev.h"

using namespace hnet;
using namespace capi;

namespace po = hnet_search_oriented;
namespace pf = hnet_search_fine;

static_assert(sizeof(hnet_photo_search_fine_opts) == sizeof(FineOpts) && offsetof(hnet_photo_search_fine_opts, n_fine) == offsetof(FineOpts, n_fine) &&
              offsetof(hnet_photo_search_fine_opts, min_score) == offsetof(FineOpts, min_score) && sizeof(hnet_photo_search_fine_part) == sizeof(FinePart) &&
              offsetof(hnet_photo_search_fine_part, flags) == offsetof(FinePart, flags) && offsetof(hnet_photo_search_fine_part, j) == offsetof(FinePart, j) &&
              offsetof(hnet_photo_search_fine_part, sx) == offsetof(FinePart, sx) && offsetof(hnet_photo_search_fine_part, n_overlap) == offsetof(FinePart, n_overlap) &&
              offsetof(hnet_photo_search_fine_part, score) == offsetof(FinePart, score) && offsetof(hnet_photo_search_fine_part, a) == offsetof(FinePart, a) &&
              offsetof(hnet_photo_search_fine_part, sa) == offsetof(FinePart, sa) && offsetof(hnet_photo_search_fine_part, pad1) == offsetof(FinePart, pad1) &&
              sizeof(hnet_photo_search_fine) == sizeof(FineRec) && offsetof(hnet_photo_search_fine, fine) == offsetof(FineRec, fine) &&
              HNET_PSF_MAX_FINE == pf::MAX_FINE && HNET_PSF_MAX_RADIUS == pf::MAX_R && (int)HNET_PSF_REFINED == pf::FINE_REFINED &&
              (int)HNET_PSF_SKIPPED == pf::FINE_SKIPPED && (int)HNET_PSF_NOTHING_SCORED == pf::FINE_NOTHING_SCORED && (int)HNET_PSF_LOW_SCORE == pf::FINE_LOW_SCORE,
              "hnet_photo_search_fine_opts / _part / hnet_photo_search_fine are the layouts of include/hnet_photo_search_fine.h");

namespace {

// both sets of thumbnails and the tables are in place on the stream: the coarse search and its winner, the fine search and its winner, ONE download
// {records [n] | fine score tables [n][n_fine]}, one synchronisation
int fine_run(hnet_ctx* c, DevTemps& t, const uint8_t* d_thumbs, const uint8_t* d_fthumbs, int ta_stride, int tb_stride, int tb_off, int n, const SearchOpts& o,
             const SearchHyp* d_hyps, int n_hyp, const FineOpts& fo, const SearchHyp* d_fine, hnet_photo_search_fine* out, double* scores_out) {
    const size_t rec_bytes = (size_t)n * sizeof(FineRec), sc_bytes = scores_out ? (size_t)n * fo.n_fine * FINE_SHIFTS * sizeof(double) : 0;
    uint8_t* d_out = nullptr;
    SearchRec* d_hrec = nullptr;
    OrientedRec* d_coarse = nullptr;
    FineEntry* d_ent = nullptr;
    HIPCHK(c, t.alloc(&d_out, rec_bytes + sc_bytes));              // (288-byte records: the tables behind them stay 8-byte aligned)
    HIPCHK(c, t.alloc(&d_hrec, (size_t)n * n_hyp));
    HIPCHK(c, t.alloc(&d_coarse, (size_t)n));
    HIPCHK(c, t.alloc(&d_ent, (size_t)n * fo.n_fine));
    std::vector<uint8_t> h_out(rec_bytes + sc_bytes);
    HIPCHK(c, launch_photo_search_oriented(d_thumbs, ta_stride, tb_stride, tb_off, 1, n, nullptr, o, d_hyps, n_hyp, d_hrec, nullptr, c->stream));
    HIPCHK(c, launch_photo_search_winner(d_hrec, d_hyps, n_hyp, n, nullptr, d_coarse, c->stream));
    HIPCHK(c, launch_photo_search_fine(d_fthumbs, ta_stride, tb_stride, tb_off, n, reinterpret_cast<const uint8_t*>(d_coarse), (int)sizeof(OrientedRec), nullptr, o, fo,
                                       d_fine, n_hyp, d_ent, scores_out ? reinterpret_cast<double*>(d_out + rec_bytes) : nullptr, c->stream));
    HIPCHK(c, launch_photo_search_fine_winner(d_ent, n, reinterpret_cast<const uint8_t*>(d_coarse), (int)sizeof(OrientedRec), nullptr, fo, d_fine, n_hyp, d_out,
                                              (int)sizeof(FineRec), (int)offsetof(FineRec, fine), true, nullptr, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_out.data(), d_out, h_out.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(out, h_out.data(), rec_bytes);
    if (scores_out) memcpy(scores_out, h_out.data() + rec_bytes, sc_bytes);
    return HNET_OK;
}

}  // namespace

namespace capi {

int photo_search_fine_check(hnet_ctx* c, const hnet_photo_search_fine_opts* fine_opts, const hnet_photo_search_hyp* fine, int n_hyp, const char* who, FineOpts& fo) {
    if (!fine_opts || !fine) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": fine_opts / fine");
    memcpy(&fo, fine_opts, sizeof fo);
    fo.pad[0] = fo.pad[1] = 0;
    if (!pf::opts_valid(fo)) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": fine_opts: 0 <= radius <= 4, 1 <= n_fine <= 9, -1 <= min_score <= 1");
    if (!pf::fine_table_valid(reinterpret_cast<const SearchHyp*>(fine), n_hyp, fo.n_fine))
        return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": fine: an entry with a non-finite a or |b[i]| > 2 * 65536");
    return HNET_OK;
}

}  // namespace capi

extern "C" {

void hnet_photo_search_fine_default_opts(hnet_photo_search_fine_opts* o) {
    if (!o) return;
    FineOpts d;
    pf::default_opts(d);
    memcpy(o, &d, sizeof d);
}

int hnet_photo_search_fine_yaw_table(double first_deg, double step_deg, int count, int n_fine, hnet_photo_search_hyp* out) {
    if (!out || count < 1 || count > po::MAX_HYP || n_fine < 1 || n_fine > pf::MAX_FINE) return 0;
    std::vector<SearchHyp> h((size_t)count * n_fine);
    if (!pf::fine_yaw_table(first_deg, step_deg, count, n_fine, h.data())) return 0;
    memcpy(out, h.data(), h.size() * sizeof(SearchHyp));
    return 1;
}

// ONE upload {img1 | img2 | table | fine table}, both thumbnails of the 2 n frames, the two stages, ONE download, one synchronisation
int hnet_op_photo_search_fine(hnet_ctx* c, const uint8_t* img1, const uint8_t* img2, int n, const hnet_photo_search_opts* opts, const hnet_photo_search_hyp* hyps,
                              int n_hyp, const hnet_photo_search_fine_opts* fine_opts, const hnet_photo_search_hyp* fine, hnet_photo_search_fine* out,
                              double* scores_out) {
    const char* who = "hnet_op_photo_search_fine";
    if (!c) return HNET_ERR_INVALID_ARG;
    if (!img1 || !img2 || !out || n < 1) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": frames / out, n >= 1");
    SearchOpts o;
    FineOpts fo;
    int rc = photo_search_check_opts(c, opts, who, o);
    if (rc == HNET_OK) rc = photo_search_check_table(c, hyps, n_hyp, who);
    if (rc == HNET_OK) rc = photo_search_fine_check(c, fine_opts, fine, n_hyp, who, fo);
    if (rc != HNET_OK) return rc;
    if (n > c->cfg.max_batch) return fail(c, HNET_ERR_CAPACITY, std::string(who) + ": n exceeds max_batch");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const size_t img = (size_t)n * NPIX, tab = (size_t)n_hyp * sizeof(SearchHyp), ftab = tab * fo.n_fine;      // (2 img is a multiple of 8: the tables are aligned)
    DevTemps t;
    uint8_t *d_in = nullptr, *d_thumbs = nullptr, *d_fthumbs = nullptr;
    HIPCHK(c, t.alloc(&d_in, 2 * img + tab + ftab));
    HIPCHK(c, t.alloc(&d_thumbs, (size_t)2 * n * THUMB_BYTES));
    HIPCHK(c, t.alloc(&d_fthumbs, (size_t)2 * n * FINE_THUMB_BYTES));
    std::vector<uint8_t> h_in(2 * img + tab + ftab);
    memcpy(h_in.data(), img1, img);
    memcpy(h_in.data() + img, img2, img);
    memcpy(h_in.data() + 2 * img, hyps, tab);
    memcpy(h_in.data() + 2 * img + tab, fine, ftab);
    HIPCHK(c, hipMemcpyAsync(d_in, h_in.data(), h_in.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_photo_thumbs(d_in, nullptr, 2 * n, 2 * n, d_thumbs, c->stream));
    HIPCHK(c, launch_photo_fine_thumbs(d_in, nullptr, 2 * n, 2 * n, d_fthumbs, c->stream));
    return fine_run(c, t, d_thumbs, d_fthumbs, 1, 1, n, n, o, reinterpret_cast<const SearchHyp*>(d_in + 2 * img), n_hyp, fo,
                    reinterpret_cast<const SearchHyp*>(d_in + 2 * img + tab), out, scores_out);       // template y, image n + y
}

// the same on the sessions' current pairs: ONE upload {pair table | table | fine table}, the thumbnails straight from the ring; nothing of the sessions' own
// tables, events or bookkeeping is touched
int hnet_sessions_photo_search_fine(hnet_sessions* s, int n, const int32_t* ids, const hnet_photo_search_opts* opts, const hnet_photo_search_hyp* hyps, int n_hyp,
                                    const hnet_photo_search_fine_opts* fine_opts, const hnet_photo_search_hyp* fine, hnet_photo_search_fine* out) {
    const char* who = "hnet_sessions_photo_search_fine";
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    if (!out) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": out");
    SearchOpts o;
    FineOpts fo;
    int rc = photo_search_check_opts(c, opts, who, o);
    if (rc == HNET_OK) rc = photo_search_check_table(c, hyps, n_hyp, who);
    if (rc == HNET_OK) rc = photo_search_fine_check(c, fine_opts, fine, n_hyp, who, fo);
    if (rc == HNET_OK) rc = sessions_check_ids(s, n, ids);
    if (rc == HNET_OK) rc = sessions_check_pairs(s, n, ids);
    if (rc != HNET_OK) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const size_t pairs = (size_t)2 * n * sizeof(int32_t), tab = (size_t)n_hyp * sizeof(SearchHyp), ftab = tab * fo.n_fine;      // (8 n bytes: the tables are aligned)
    std::vector<uint8_t> h_in(pairs + tab + ftab);
    for (int i = 0; i < n; i++) sessions_pair(s, ids[i], reinterpret_cast<int32_t*>(h_in.data()) + 2 * i);
    memcpy(h_in.data() + pairs, hyps, tab);
    memcpy(h_in.data() + pairs + tab, fine, ftab);
    DevTemps t;
    uint8_t *d_in = nullptr, *d_thumbs = nullptr, *d_fthumbs = nullptr;
    HIPCHK(c, t.alloc(&d_in, pairs + tab + ftab));
    HIPCHK(c, t.alloc(&d_thumbs, (size_t)2 * n * THUMB_BYTES));
    HIPCHK(c, t.alloc(&d_fthumbs, (size_t)2 * n * FINE_THUMB_BYTES));
    HIPCHK(c, hipMemcpyAsync(d_in, h_in.data(), h_in.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_photo_thumbs(s->ring, reinterpret_cast<const int32_t*>(d_in), 2 * s->n, 2 * n, d_thumbs, c->stream));
    HIPCHK(c, launch_photo_fine_thumbs(s->ring, reinterpret_cast<const int32_t*>(d_in), 2 * s->n, 2 * n, d_fthumbs, c->stream));
    return fine_run(c, t, d_thumbs, d_fthumbs, 2, 2, 1, n, o, reinterpret_cast<const SearchHyp*>(d_in + pairs), n_hyp, fo,
                    reinterpret_cast<const SearchHyp*>(d_in + pairs + tab), out, nullptr);           // template 2 y, image 2 y + 1
}

}  // extern "C"
