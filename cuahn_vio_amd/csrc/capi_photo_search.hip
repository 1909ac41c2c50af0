// capi_photo_search.hip — hnet_photo_search_*, hnet_op_photo_search and hnet_sessions_photo_search of include/hnet.h (photo_search_dev.h,
// csrc/kernels_photo_search.hip): the coarse search over integer translations between the level-3 thumbnails of two frames.  Both calls own
// their thumbnails, records and score tables as device temporaries: nothing of the context's pyramid scratch, events or timings is touched.  The
// relocalisation that runs the same kernels over a session's keyframes is capi_keyframe.hip's.
#include "sessions_internal.h"
#include "photo_search_dev.h"

using namespace hnet;
using namespace capi;

namespace ps = hnet_search;

static_assert(sizeof(hnet_photo_search) == sizeof(SearchRec) && offsetof(hnet_photo_search, dx2) == offsetof(SearchRec, dx2) &&
              offsetof(hnet_photo_search, flags) == offsetof(SearchRec, flags) && offsetof(hnet_photo_search, second) == offsetof(SearchRec, second) &&
              offsetof(hnet_photo_search, sbb) == offsetof(SearchRec, sbb) && sizeof(hnet_photo_search_opts) == sizeof(SearchOpts) &&
              offsetof(hnet_photo_search_opts, min_overlap) == offsetof(SearchOpts, min_overlap) &&
              offsetof(hnet_photo_search_opts, min_margin) == offsetof(SearchOpts, min_margin), "hnet_photo_search / _opts are the layouts of include/hnet_photo_search.h");
static_assert((int)HNET_PS_FOUND == ps::FOUND && (int)HNET_PS_NO_TEXTURE == ps::NO_TEXTURE && (int)HNET_PS_LOW_SCORE == ps::LOW_SCORE &&
              (int)HNET_PS_AMBIGUOUS == ps::AMBIGUOUS && HNET_PS_SHIFTS_X == ps::NSX && HNET_PS_SHIFTS_Y == ps::NSY, "HNET_PS_* are the header's");

namespace capi {

int photo_search_check_opts(hnet_ctx* c, const hnet_photo_search_opts* opts, const char* who, SearchOpts& o) {
    if (!opts) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": opts");
    memcpy(&o, opts, sizeof o);
    if (!ps::opts_valid(o))
        return fail(c, HNET_ERR_INVALID_ARG,
                    std::string(who) + ": opts: 0 <= radius_x <= 30, 0 <= radius_y <= 20, 16 <= min_overlap <= 1120, -1 <= min_score <= 1, 0 <= min_margin <= 2");
    o.pad = 0;
    return HNET_OK;
}

}  // namespace capi

namespace {

// the thumbnails are in place on the stream: the search, ONE download {records [n] | score tables [n]}, one synchronisation
int search_run(hnet_ctx* c, DevTemps& t, const uint8_t* d_thumbs, int ta_stride, int tb_stride, int tb_off, int n, const SearchOpts& o, hnet_photo_search* out,
               double* scores_out) {
    const size_t rec_bytes = (size_t)n * sizeof(SearchRec), sc_bytes = scores_out ? (size_t)n * SEARCH_SHIFTS * sizeof(double) : 0;
    uint8_t* d_out = nullptr;
    HIPCHK(c, t.alloc(&d_out, rec_bytes + sc_bytes));              // (96-byte records: the tables behind them stay 8-byte aligned)
    std::vector<uint8_t> h_out(rec_bytes + sc_bytes);
    HIPCHK(c, launch_photo_search(d_thumbs, ta_stride, tb_stride, tb_off, 1, n, nullptr, o, reinterpret_cast<SearchRec*>(d_out),
                                  scores_out ? reinterpret_cast<double*>(d_out + rec_bytes) : nullptr, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_out.data(), d_out, h_out.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(out, h_out.data(), rec_bytes);
    if (scores_out) memcpy(scores_out, h_out.data() + rec_bytes, sc_bytes);
    return HNET_OK;
}

}  // namespace

extern "C" {

void hnet_photo_search_default_opts(hnet_photo_search_opts* o) {
    if (!o) return;
    SearchOpts d;
    ps::default_opts(d);
    memcpy(o, &d, sizeof d);
}

// ONE upload {img1 | img2}, the thumbnails of the 2 n frames, the search, ONE download, one synchronisation
int hnet_op_photo_search(hnet_ctx* c, const uint8_t* img1, const uint8_t* img2, int n, const hnet_photo_search_opts* opts, hnet_photo_search* out,
                         double* scores_out) {
    const char* who = "hnet_op_photo_search";
    if (!c) return HNET_ERR_INVALID_ARG;
    if (!img1 || !img2 || !out || n < 1) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": frames / out, n >= 1");
    SearchOpts o;
    const int rc = photo_search_check_opts(c, opts, who, o);
    if (rc != HNET_OK) return rc;
    if (n > c->cfg.max_batch) return fail(c, HNET_ERR_CAPACITY, std::string(who) + ": n exceeds max_batch");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const size_t img = (size_t)n * NPIX;
    DevTemps t;
    uint8_t *d_in = nullptr, *d_thumbs = nullptr;
    HIPCHK(c, t.alloc(&d_in, 2 * img));
    HIPCHK(c, t.alloc(&d_thumbs, (size_t)2 * n * THUMB_BYTES));
    std::vector<uint8_t> h_in(2 * img);
    memcpy(h_in.data(), img1, img);
    memcpy(h_in.data() + img, img2, img);
    HIPCHK(c, hipMemcpyAsync(d_in, h_in.data(), 2 * img, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_photo_thumbs(d_in, nullptr, 2 * n, 2 * n, d_thumbs, c->stream));
    return search_run(c, t, d_thumbs, 1, 1, n, n, o, out, scores_out);       // template y, image n + y
}

// the same on the sessions' current pairs: ONE upload of the pair table, the thumbnails straight from the ring; nothing of the sessions' own tables,
// events or bookkeeping is touched
int hnet_sessions_photo_search(hnet_sessions* s, int n, const int32_t* ids, const hnet_photo_search_opts* opts, hnet_photo_search* out) {
    const char* who = "hnet_sessions_photo_search";
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    if (!out) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": out");
    SearchOpts o;
    int rc = photo_search_check_opts(c, opts, who, o);
    if (rc == HNET_OK) rc = sessions_check_ids(s, n, ids);
    if (rc == HNET_OK) rc = sessions_check_pairs(s, n, ids);
    if (rc != HNET_OK) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    std::vector<int32_t> h_in((size_t)2 * n);
    for (int i = 0; i < n; i++) sessions_pair(s, ids[i], h_in.data() + 2 * i);
    DevTemps t;
    int32_t* d_in = nullptr;
    uint8_t* d_thumbs = nullptr;
    HIPCHK(c, t.alloc(&d_in, (size_t)2 * n));
    HIPCHK(c, t.alloc(&d_thumbs, (size_t)2 * n * THUMB_BYTES));
    HIPCHK(c, hipMemcpyAsync(d_in, h_in.data(), h_in.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_photo_thumbs(s->ring, d_in, 2 * s->n, 2 * n, d_thumbs, c->stream));
    return search_run(c, t, d_thumbs, 2, 2, 1, n, o, out, nullptr);           // template 2 y, image 2 y + 1
}

}  // extern "C"
