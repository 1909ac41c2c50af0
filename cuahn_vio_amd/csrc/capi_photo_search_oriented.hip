// capi_photo_search_oriented.hip — hnet_photo_search_make_hyp / _yaw_table, hnet_op_photo_search_oriented and hnet_sessions_photo_search_oriented of
// include/hnet.h (photo_search_oriented_dev.h, csrc/kernels_photo_search_oriented.hip): the coarse search under a table of orientation
// hypotheses.  Both calls own their thumbnails, table, records and score tables as device temporaries: nothing of the context's pyramid scratch, events
// or timings is touched.  The relocalisation that runs the same kernels over a session's keyframes is capi_keyframe.hip's.
#include "sessions_internal.h"
#include "photo_search_oriented_dev.h"

using namespace hnet;
using namespace capi;

namespace po = hnet_search_oriented;

static_assert(sizeof(hnet_photo_search_hyp) == sizeof(SearchHyp) && offsetof(hnet_photo_search_hyp, b) == offsetof(SearchHyp, b) &&
              sizeof(hnet_photo_search_oriented) == sizeof(OrientedRec) && offsetof(hnet_photo_search_oriented, hyp) == offsetof(OrientedRec, hyp) &&
              offsetof(hnet_photo_search_oriented, n_scored) == offsetof(OrientedRec, n_scored) && offsetof(hnet_photo_search_oriented, hyp2) == offsetof(OrientedRec, hyp2) &&
              offsetof(hnet_photo_search_oriented, score2) == offsetof(OrientedRec, score2) && offsetof(hnet_photo_search_oriented, a) == offsetof(OrientedRec, a) &&
              offsetof(hnet_photo_search_oriented, pad) == offsetof(OrientedRec, pad) && HNET_PS_MAX_HYP == po::MAX_HYP && HNET_PS_DEFAULT_HYP == po::DEFAULT_COUNT,
              "hnet_photo_search_hyp / _oriented are the layouts of include/hnet_photo_search_oriented.h");

namespace {

// the thumbnails and the table are in place on the stream: the search, the winner, ONE download {records [n] | score tables [n][n_hyp]}, one synchronisation
int search_run(hnet_ctx* c, DevTemps& t, const uint8_t* d_thumbs, int ta_stride, int tb_stride, int tb_off, int n, const SearchOpts& o, const SearchHyp* d_hyps,
               int n_hyp, hnet_photo_search_oriented* out, double* scores_out) {
    const size_t rec_bytes = (size_t)n * sizeof(OrientedRec), sc_bytes = scores_out ? (size_t)n * n_hyp * SEARCH_SHIFTS * sizeof(double) : 0;
    uint8_t* d_out = nullptr;
    SearchRec* d_hrec = nullptr;
    HIPCHK(c, t.alloc(&d_out, rec_bytes + sc_bytes));              // (160-byte records: the tables behind them stay 8-byte aligned)
    HIPCHK(c, t.alloc(&d_hrec, (size_t)n * n_hyp));
    std::vector<uint8_t> h_out(rec_bytes + sc_bytes);
    HIPCHK(c, launch_photo_search_oriented(d_thumbs, ta_stride, tb_stride, tb_off, 1, n, nullptr, o, d_hyps, n_hyp, d_hrec,
                                           scores_out ? reinterpret_cast<double*>(d_out + rec_bytes) : nullptr, c->stream));
    HIPCHK(c, launch_photo_search_winner(d_hrec, d_hyps, n_hyp, n, nullptr, reinterpret_cast<OrientedRec*>(d_out), c->stream));
    HIPCHK(c, hipMemcpyAsync(h_out.data(), d_out, h_out.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(out, h_out.data(), rec_bytes);
    if (scores_out) memcpy(scores_out, h_out.data() + rec_bytes, sc_bytes);
    return HNET_OK;
}

}  // namespace

namespace capi {

int photo_search_check_table(hnet_ctx* c, const hnet_photo_search_hyp* hyps, int n_hyp, const char* who) {
    if (!hyps || n_hyp < 1 || n_hyp > po::MAX_HYP) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": hyps, 1 <= n_hyp <= 64");
    if (!po::table_valid(reinterpret_cast<const SearchHyp*>(hyps), n_hyp))
        return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": hyps: an entry with a non-finite a or |b[i]| > 2 * 65536");
    return HNET_OK;
}

}  // namespace capi

extern "C" {

int hnet_photo_search_make_hyp(double angle_rad, double scale, hnet_photo_search_hyp* out) {
    SearchHyp h;
    if (!out || !po::make_hyp(angle_rad, scale, h)) return 0;
    memcpy(out, &h, sizeof h);
    return 1;
}

int hnet_photo_search_yaw_table(double first_deg, double step_deg, int count, hnet_photo_search_hyp* out) {
    SearchHyp h[po::MAX_HYP];
    if (!out || !po::yaw_table(first_deg, step_deg, count, h)) return 0;
    memcpy(out, h, (size_t)count * sizeof(SearchHyp));
    return 1;
}

int hnet_photo_search_default_yaw_table(hnet_photo_search_hyp* out) {
    return hnet_photo_search_yaw_table(po::DEFAULT_FIRST_DEG, po::DEFAULT_STEP_DEG, po::DEFAULT_COUNT, out) ? po::DEFAULT_COUNT : 0;
}

// ONE upload {img1 | img2 | table}, the thumbnails of the 2 n frames, the search, the winner, ONE download, one synchronisation
int hnet_op_photo_search_oriented(hnet_ctx* c, const uint8_t* img1, const uint8_t* img2, int n, const hnet_photo_search_opts* opts,
                                  const hnet_photo_search_hyp* hyps, int n_hyp, hnet_photo_search_oriented* out, double* scores_out) {
    const char* who = "hnet_op_photo_search_oriented";
    if (!c) return HNET_ERR_INVALID_ARG;
    if (!img1 || !img2 || !out || n < 1) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": frames / out, n >= 1");
    SearchOpts o;
    int rc = photo_search_check_opts(c, opts, who, o);
    if (rc == HNET_OK) rc = photo_search_check_table(c, hyps, n_hyp, who);
    if (rc != HNET_OK) return rc;
    if (n > c->cfg.max_batch) return fail(c, HNET_ERR_CAPACITY, std::string(who) + ": n exceeds max_batch");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const size_t img = (size_t)n * NPIX, tab = (size_t)n_hyp * sizeof(SearchHyp);      // (2 img is a multiple of 8: the table behind the frames is aligned)
    DevTemps t;
    uint8_t *d_in = nullptr, *d_thumbs = nullptr;
    HIPCHK(c, t.alloc(&d_in, 2 * img + tab));
    HIPCHK(c, t.alloc(&d_thumbs, (size_t)2 * n * THUMB_BYTES));
    std::vector<uint8_t> h_in(2 * img + tab);
    memcpy(h_in.data(), img1, img);
    memcpy(h_in.data() + img, img2, img);
    memcpy(h_in.data() + 2 * img, hyps, tab);
    HIPCHK(c, hipMemcpyAsync(d_in, h_in.data(), h_in.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_photo_thumbs(d_in, nullptr, 2 * n, 2 * n, d_thumbs, c->stream));
    return search_run(c, t, d_thumbs, 1, 1, n, n, o, reinterpret_cast<const SearchHyp*>(d_in + 2 * img), n_hyp, out, scores_out);       // template y, image n + y
}

// the same on the sessions' current pairs: ONE upload {pair table | table}, the thumbnails straight from the ring; nothing of the sessions' own tables,
// events or bookkeeping is touched
int hnet_sessions_photo_search_oriented(hnet_sessions* s, int n, const int32_t* ids, const hnet_photo_search_opts* opts, const hnet_photo_search_hyp* hyps,
                                        int n_hyp, hnet_photo_search_oriented* out) {
    const char* who = "hnet_sessions_photo_search_oriented";
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    if (!out) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": out");
    SearchOpts o;
    int rc = photo_search_check_opts(c, opts, who, o);
    if (rc == HNET_OK) rc = photo_search_check_table(c, hyps, n_hyp, who);
    if (rc == HNET_OK) rc = sessions_check_ids(s, n, ids);
    if (rc == HNET_OK) rc = sessions_check_pairs(s, n, ids);
    if (rc != HNET_OK) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const size_t pairs = (size_t)2 * n * sizeof(int32_t), tab = (size_t)n_hyp * sizeof(SearchHyp);      // (8 n bytes: the table behind the pairs is aligned)
    std::vector<uint8_t> h_in(pairs + tab);
    for (int i = 0; i < n; i++) sessions_pair(s, ids[i], reinterpret_cast<int32_t*>(h_in.data()) + 2 * i);
    memcpy(h_in.data() + pairs, hyps, tab);
    DevTemps t;
    uint8_t *d_in = nullptr, *d_thumbs = nullptr;
    HIPCHK(c, t.alloc(&d_in, pairs + tab));
    HIPCHK(c, t.alloc(&d_thumbs, (size_t)2 * n * THUMB_BYTES));
    HIPCHK(c, hipMemcpyAsync(d_in, h_in.data(), h_in.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_photo_thumbs(s->ring, reinterpret_cast<const int32_t*>(d_in), 2 * s->n, 2 * n, d_thumbs, c->stream));
    return search_run(c, t, d_thumbs, 2, 2, 1, n, o, reinterpret_cast<const SearchHyp*>(d_in + pairs), n_hyp, out, nullptr);           // template 2 y, image 2 y + 1
}

}  // extern "C"
