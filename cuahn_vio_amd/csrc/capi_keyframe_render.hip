// capi_keyframe_render.hip — hnet_keyframe_render_fit_view, hnet_op_keyframe_render, hnet_sessions_enable_keyframe_render and
// hnet_sessions_keyframe_render of include/hnet.h (keyframe_render_dev.h, csrc/kernels_keyframe_render.hip): a keyframe map rendered into a
// view with its cover image and seam statistics.  The operator-level call owns its buffers as device temporaries.  The sessions call reads the map and
// the states of the keyframe store (keyframes_internal.h) and writes only buffers of its own, allocated by its enable: additive, a store whose render
// was never enabled holds a null pointer and allocates and launches nothing here.
#include "keyframes_internal.h"

#include <memory>

using namespace hnet;
using namespace capi;

namespace kr = hnet_keyframe_render;

static_assert(sizeof(hnet_keyframe_render_rec) == sizeof(RenderRec) && offsetof(hnet_keyframe_render_rec, n_covered) == offsetof(RenderRec, c.n_covered) &&
              offsetof(hnet_keyframe_render_rec, n) == offsetof(RenderRec, c.n) && offsetof(hnet_keyframe_render_rec, sse) == offsetof(RenderRec, c.sse) &&
              offsetof(hnet_keyframe_render_rec, used_mask) == offsetof(RenderRec, used_mask) &&
              offsetof(hnet_keyframe_render_rec, skipped_mask) == offsetof(RenderRec, skipped_mask) && sizeof(hnet_keyframe_render_opts) == sizeof(RenderOpts) &&
              offsetof(hnet_keyframe_render_opts, mode) == offsetof(RenderOpts, mode),
              "hnet_keyframe_render_rec / _opts are the layouts of include/hnet_keyframe_render.h");
static_assert((int)HNET_RENDER_FEWEST_LINKS == kr::FEWEST_LINKS && (int)HNET_RENDER_NEWEST == kr::NEWEST && (int)HNET_RENDER_MEAN == kr::MEAN &&
              HNET_RENDER_MAX_DIM == kr::MAX_DIM, "HNET_RENDER_* are the header's");

namespace {

// the render of a store: sized at its enable for max_batch B and views up to max_w x max_h
struct KeyRender : KeyLayer {
    int max_w = 0, max_h = 0;
    uint8_t* d_in = nullptr;                   // device: a call's table {ids [n] i32, padded to 8 bytes | views [n][9] f64}
    RenderTab* tab = nullptr;                  // device [B]
    uint8_t* d_out = nullptr;                  // device: a call's results {records [n] | images [n][h][w] | covers [n][h][w]}, packed for ONE download
    uint8_t *pin_in = nullptr, *pin_out = nullptr;     // pinned: the same two blocks
};

constexpr size_t ids_bytes(int n) { return ((size_t)n * sizeof(int32_t) + 7) & ~(size_t)7; }
constexpr size_t in_bytes(int n) { return ids_bytes(n) + (size_t)n * 9 * sizeof(double); }
static_assert(KeyUpload(1, KeyUpload::VIEW).view == ids_bytes(1) && KeyUpload(1, KeyUpload::VIEW).entry == in_bytes(1),
              "the operator-level block begins with the table of a sessions call of one");
size_t out_bytes(int n, int w, int h) { return (size_t)n * (sizeof(RenderRec) + 2 * (size_t)w * h); }

// o <- *opts with its pad zeroed, or the context's error; max_w, max_h: the largest view the caller's buffers hold
int check_opts(hnet_ctx* c, const hnet_keyframe_render_opts* opts, int max_w, int max_h, const char* who, RenderOpts& o) {
    memcpy(&o, opts, sizeof o);
    o.pad = 0;
    if (!kr::opts_valid(o) || o.width > max_w || o.height > max_h)
        return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": opts: mode 0 .. 2, width and height from 1 to the maximum (HNET_RENDER_MAX_DIM, or what was enabled)");
    return HNET_OK;
}

}  // namespace

extern "C" {

int hnet_keyframe_render_fit_view(const hnet_keyframe_map_entry* entries, int capacity, int width, int height, double margin_px, double* h_origin_view) {
    if (!entries || !h_origin_view || capacity < 1 || capacity > kr::MAX_ENTRIES || width < 1 || height < 1) return 0;
    return kr::render_fit_view(reinterpret_cast<const MapEntry*>(entries), capacity, width, height, margin_px, h_origin_view) ? 1 : 0;
}

// ONE upload {id 0 | view | entries [m] | images [m]}, the two launches, ONE download {record | image | cover}, one synchronisation
int hnet_op_keyframe_render(hnet_ctx* c, int m, const uint8_t* images, const hnet_keyframe_map_entry* entries, const double* h_origin_view,
                            const hnet_keyframe_render_opts* opts, uint8_t* out_img, uint8_t* out_cover, hnet_keyframe_render_rec* rec) {
    const char* who = "hnet_op_keyframe_render";
    if (!c) return HNET_ERR_INVALID_ARG;
    if (!images || !entries || !h_origin_view || !opts || !out_img || !out_cover || !rec)
        return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": images / entries / h_origin_view / opts / out_img / out_cover / rec");
    if (m < 1 || m > kr::MAX_ENTRIES) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": 1 <= m <= 8");
    RenderOpts o;
    const int rc = check_opts(c, opts, kr::MAX_DIM, kr::MAX_DIM, who, o);
    if (rc != HNET_OK) return rc;
    if (!all_finite(h_origin_view, 9)) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": h_origin_view is not finite");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const KeyUpload up(m, KeyUpload::VIEW | KeyUpload::IMAGES);       // (the table as the sessions call lays it out, then the entries and the images)
    const size_t px = (size_t)o.width * o.height, out_total = out_bytes(1, o.width, o.height);
    std::vector<uint8_t> h_in(up.total, 0), h_out(out_total);
    memcpy(h_in.data() + up.view, h_origin_view, 9 * sizeof(double));
    memcpy(h_in.data() + up.entry, entries, (size_t)m * sizeof(MapEntry));
    memcpy(h_in.data() + up.images, images, (size_t)m * NPIX);
    DevTemps t;
    uint8_t *d_in = nullptr, *d_out = nullptr;
    RenderTab* d_tab = nullptr;
    HIPCHK(c, t.alloc(&d_in, up.total));
    HIPCHK(c, t.alloc(&d_out, out_total));
    HIPCHK(c, t.alloc(&d_tab, 1));
    const RenderSource src{d_in + up.images, reinterpret_cast<const MapEntry*>(d_in + up.entry), nullptr, 1, m};
    RenderRec* d_rec = reinterpret_cast<RenderRec*>(d_out);
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(d_in, h_in.data(), up.total, hipMemcpyHostToDevice, st));
    HIPCHK(c, launch_keyframe_render_setup(reinterpret_cast<const int32_t*>(d_in), 1, src, reinterpret_cast<const double*>(d_in + up.view), d_tab, d_rec, st));
    HIPCHK(c, launch_keyframe_render(reinterpret_cast<const int32_t*>(d_in), 1, src, d_tab, o, d_out + sizeof(RenderRec), d_out + sizeof(RenderRec) + px, d_rec, st));
    HIPCHK(c, hipMemcpyAsync(h_out.data(), d_out, out_total, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    memcpy(rec, h_out.data(), sizeof(RenderRec));
    memcpy(out_img, h_out.data() + sizeof(RenderRec), px);
    memcpy(out_cover, h_out.data() + sizeof(RenderRec) + px, px);
    return HNET_OK;
}

int hnet_sessions_enable_keyframe_render(hnet_sessions* s, int max_width, int max_height) {
    const char* who = "hnet_sessions_enable_keyframe_render";
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    hnet_keyframes* k = s->kf;
    if (!k || !k->map) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": the keyframe map is not enabled (hnet_sessions_enable_keyframe_map)");
    if (k->render) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": the keyframe render is already enabled");
    if (max_width < 1 || max_width > kr::MAX_DIM || max_height < 1 || max_height > kr::MAX_DIM)
        return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": 1 <= max_width, max_height <= HNET_RENDER_MAX_DIM");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const int B = c->cfg.max_batch;
    auto r = std::make_unique<KeyRender>();
    r->max_w = max_width;
    r->max_h = max_height;
    hipError_t e = r->mem.alloc(&r->d_in, in_bytes(B));
    if (e == hipSuccess) e = r->mem.alloc(&r->tab, (size_t)B);
    if (e == hipSuccess) e = r->mem.alloc(&r->d_out, out_bytes(B, max_width, max_height));
    if (e == hipSuccess) e = r->mem.alloc_pinned(&r->pin_in, in_bytes(B));
    if (e == hipSuccess) e = r->mem.alloc_pinned(&r->pin_out, out_bytes(B, max_width, max_height));
    if (e != hipSuccess) return fail(c, HNET_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    k->render = r.release();
    return HNET_OK;
}

// ONE upload {ids | views}, the two launches inside the store's events, ONE download {records | images | covers}, one synchronisation
int hnet_sessions_keyframe_render(hnet_sessions* s, int n, const int32_t* ids, const double* h_origin_view, const hnet_keyframe_render_opts* opts,
                                  uint8_t* out_img, uint8_t* out_cover, hnet_keyframe_render_rec* out) {
    const char* who = "hnet_sessions_keyframe_render";
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    hnet_keyframes* k = s->kf;
    if (!k || !k->map || !k->render)
        return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": the keyframe render is not enabled (hnet_sessions_enable_keyframe_render)");
    KeyRender* r = static_cast<KeyRender*>(k->render);
    if (!opts || !out_img || !out_cover || !out) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": opts / out_img / out_cover / out");
    RenderOpts o;
    int rc = check_opts(c, opts, r->max_w, r->max_h, who, o);
    if (rc != HNET_OK) return rc;
    if ((rc = sessions_check_ids(s, n, ids)) != HNET_OK) return rc;
    if (h_origin_view) {
        if (!all_finite(h_origin_view, (size_t)n * 9)) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": h_origin_view is not finite");
    } else if ((rc = check_listed(s, n, ids, who, true)) != HNET_OK) {
        return rc;
    }
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    int32_t* h_ids = reinterpret_cast<int32_t*>(r->pin_in);
    for (int i = 0; i < n; i++) h_ids[i] = ids[i];
    if (n & 1) h_ids[n] = 0;                                           // (the padding is uploaded too)
    const size_t head = ids_bytes(n), up = head + (h_origin_view ? (size_t)n * 9 * sizeof(double) : 0);
    if (h_origin_view) memcpy(r->pin_in + head, h_origin_view, (size_t)n * 9 * sizeof(double));
    const size_t px = (size_t)n * o.width * o.height, recs = (size_t)n * sizeof(RenderRec), total = recs + 2 * px;
    const int32_t* d_ids = reinterpret_cast<const int32_t*>(r->d_in);
    RenderRec* d_rec = reinterpret_cast<RenderRec*>(r->d_out);
    const RenderSource src = render_source(k);
    hipStream_t st = c->stream;
    if ((rc = begin_call(c, k, r->d_in, r->pin_in, up)) != HNET_OK) return rc;
    HIPCHK(c, launch_keyframe_render_setup(d_ids, n, src, h_origin_view ? reinterpret_cast<const double*>(r->d_in + head) : nullptr, r->tab, d_rec, st));
    HIPCHK(c, launch_keyframe_render(d_ids, n, src, r->tab, o, r->d_out + recs, r->d_out + recs + px, d_rec, st));
    if ((rc = finish_call(c, k, r->d_out, r->pin_out, nullptr, total)) != HNET_OK) return rc;
    memcpy(out, r->pin_out, recs);
    memcpy(out_img, r->pin_out + recs, px);
    memcpy(out_cover, r->pin_out + recs + px, px);
    return HNET_OK;
}

}  // extern "C"
