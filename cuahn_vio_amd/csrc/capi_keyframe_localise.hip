// capi_keyframe_localise.hip — hnet_keyframe_localise_default_opts and hnet_op_keyframe_localise of include/hnet.h (keyframe_localise_dev.h,
// csrc/kernels_keyframe_localise.hip): a camera localised against its rendered keyframe map.  The operator-level call owns its buffers as
// device temporaries and runs the unchanged render (keyframe_render_dev.h) and the masked alignment (photo_masked_dev.h) between its two small kernels.
// The sessions call reads the map, the states and the alignment scratch of the keyframe store (keyframes_internal.h) and owns its templates, tables and
// records, allocated by its enable.
#include "keyframes_internal.h"
#include "keyframe_localise_dev.h"

#include <memory>

using namespace hnet;
using namespace capi;

namespace kl = hnet_localise;

static_assert(sizeof(hnet_keyframe_localise) == sizeof(LocaliseRec) && offsetof(hnet_keyframe_localise, h_origin_before) == offsetof(LocaliseRec, h_origin_before) &&
              offsetof(hnet_keyframe_localise, correction_px) == offsetof(LocaliseRec, correction_px) && offsetof(hnet_keyframe_localise, cover) == offsetof(LocaliseRec, cover) &&
              offsetof(hnet_keyframe_localise, used_mask) == offsetof(LocaliseRec, used_mask) && offsetof(hnet_keyframe_localise, flags) == offsetof(LocaliseRec, flags) &&
              sizeof(hnet_keyframe_localise_opts) == sizeof(LocaliseOpts) && offsetof(hnet_keyframe_localise_opts, mode) == offsetof(LocaliseOpts, mode) &&
              offsetof(hnet_keyframe_localise_opts, min_cover) == offsetof(LocaliseOpts, min_cover) && offsetof(hnet_keyframe_localise_opts, apply) == offsetof(LocaliseOpts, apply),
              "hnet_keyframe_localise / _opts are the layouts of include/hnet_keyframe_localise.h");
static_assert((int)HNET_LOC_NO_MAP == kl::LOC_NO_MAP && (int)HNET_LOC_LOW_COVER == kl::LOC_LOW_COVER && (int)HNET_LOC_STOPPED == kl::LOC_STOPPED &&
              (int)HNET_LOC_MSE_ABOVE_MAX == kl::LOC_MSE_ABOVE_MAX && (int)HNET_LOC_NON_FINITE == kl::LOC_NON_FINITE && (int)HNET_LOC_LOW_OVERLAP == kl::LOC_LOW_OVERLAP &&
              (int)HNET_LOC_SHIFT_ABOVE_MAX == kl::LOC_SHIFT_ABOVE_MAX && (int)HNET_LOC_CHAIN == kl::LOC_CHAIN && (int)HNET_LOC_LOCALISED == kl::LOC_LOCALISED,
              "HNET_LOC_* are the header's");
static_assert(sizeof(LocaliseRec) % 16 == 0, "the template behind the record stays 16-byte aligned");

namespace {

// the localise of a store: sized at its enable for max_batch B
struct KeyLocalise : KeyLayer {
    int32_t* d_in = nullptr;                   // device: a call's table {ids [n] | curr ring slot [n]}
    RenderTab* tab = nullptr;                  // device [B]
    RenderRec* rrec = nullptr;                 // device [B]
    uint8_t *tmpl = nullptr, *cover = nullptr; // device [B][NPIX] each: the templates and their cover images (the masks)
    uint8_t* mpyr = nullptr;                   // device [B][PYR_BYTES]
    int32_t* n_mask = nullptr;                 // device [B][N_MASK]
    LocaliseRec* d_out = nullptr;              // device [B]
    int32_t* pin_in = nullptr;                 // pinned: the table
    LocaliseRec* pin_out = nullptr;            // pinned: the records
};

// o <- *opts checked, or the context's error
int check_opts(hnet_ctx* c, const hnet_keyframe_localise_opts* opts, const char* who, LocaliseOpts& o) {
    const int rc = photo_robust_check_opts(c, &opts->align, who);
    if (rc != HNET_OK) return rc;
    memcpy(&o, opts, sizeof o);
    o.pad = 0;
    if (!kl::opts_valid(o))
        return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": opts: 1 <= levels <= 4, mode 0 .. 2, min_cover and min_overlap in 0 .. 1, max_mse and max_shift_px >= 0 and "
                                                                "finite, apply 0 / 1");
    return HNET_OK;
}

}  // namespace

extern "C" {

void hnet_keyframe_localise_default_opts(hnet_keyframe_localise_opts* o) {
    if (!o) return;
    LocaliseOpts d;
    kl::default_opts(d);
    memcpy(o, &d, sizeof d);
}

// ONE upload {id 0 | view | entries [m] | images [m] | curr}, {render setup, render, start, mask pyramid + masked alignment, decide}, ONE download
// {record | template | cover}, one synchronisation
int hnet_op_keyframe_localise(hnet_ctx* c, int m, const uint8_t* images, const hnet_keyframe_map_entry* entries, const double* h_origin_pred, const uint8_t* curr,
                              const hnet_keyframe_localise_opts* opts, hnet_keyframe_localise* out, uint8_t* out_template, uint8_t* out_cover) {
    const char* who = "hnet_op_keyframe_localise";
    if (!c) return HNET_ERR_INVALID_ARG;
    if (!images || !entries || !h_origin_pred || !curr || !opts || !out)
        return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": images / entries / h_origin_pred / curr / opts / out");
    if (m < 1 || m > RENDER_MAX) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": 1 <= m <= 8");
    LocaliseOpts o;
    const int rc = check_opts(c, opts, who, o);
    if (rc != HNET_OK) return rc;
    if (!all_finite(h_origin_pred, 9)) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": h_origin_pred is not finite");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const KeyUpload up(m, KeyUpload::VIEW | KeyUpload::IMAGES | KeyUpload::FRAME);
    const size_t out_total = sizeof(LocaliseRec) + 2 * (size_t)NPIX;
    std::vector<uint8_t> h_in(up.total, 0), h_out(out_total);
    memcpy(h_in.data() + up.view, h_origin_pred, 9 * sizeof(double));
    memcpy(h_in.data() + up.entry, entries, (size_t)m * sizeof(MapEntry));
    memcpy(h_in.data() + up.images, images, (size_t)m * NPIX);
    memcpy(h_in.data() + up.frame, curr, NPIX);
    const size_t pyr = (size_t)c->cfg.max_batch * PYR_BYTES;
    if (o.levels > 1)
        if (const int e = ensure_pyr_scratch(c); e != HNET_OK) return e;
    DevTemps t;
    uint8_t *d_in = nullptr, *d_out = nullptr, *d_mpyr = nullptr;
    RenderTab* d_tab = nullptr;
    RenderRec* d_rrec = nullptr;
    float* d_x0 = nullptr;
    int32_t* d_n_mask = nullptr;
    RobustSums* d_part = nullptr;
    RobustWork* d_work = nullptr;
    RobustRec* d_arec = nullptr;
    RobustStart* d_start = nullptr;
    HIPCHK(c, t.alloc(&d_in, up.total));
    HIPCHK(c, t.alloc(&d_out, out_total));
    HIPCHK(c, t.alloc(&d_tab, 1));
    HIPCHK(c, t.alloc(&d_rrec, 1));
    HIPCHK(c, t.alloc(&d_x0, 8));
    HIPCHK(c, t.alloc(&d_mpyr, (size_t)PYR_BYTES));
    HIPCHK(c, t.alloc(&d_n_mask, (size_t)N_MASK));
    HIPCHK(c, t.alloc(&d_part, (size_t)PHOTO_SLICES));
    HIPCHK(c, t.alloc(&d_work, 1));
    HIPCHK(c, t.alloc(&d_arec, (size_t)o.levels));
    HIPCHK(c, t.alloc(&d_start, 1));
    const RenderSource src{d_in + up.images, reinterpret_cast<const MapEntry*>(d_in + up.entry), nullptr, 1, m};
    const int32_t* d_id = reinterpret_cast<const int32_t*>(d_in);
    const RenderOpts ro{IMG_W, IMG_H, o.mode, 0};
    RobustOpts ao;
    memcpy(&ao, &o.align, sizeof ao);
    uint8_t *d_tmpl = d_out + sizeof(LocaliseRec), *d_cover = d_tmpl + NPIX;
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(d_in, h_in.data(), up.total, hipMemcpyHostToDevice, st));
    HIPCHK(c, launch_keyframe_render_setup(d_id, 1, src, reinterpret_cast<const double*>(d_in + up.view), d_tab, d_rrec, st));
    HIPCHK(c, launch_keyframe_render(d_id, 1, src, d_tab, ro, d_tmpl, d_cover, d_rrec, st));
    HIPCHK(c, launch_keyframe_localise_start(d_rrec, 1, o, d_x0, st));
    HIPCHK(c, launch_photo_align_masked(d_tmpl, d_cover, d_in + up.frame, 1, d_x0, ao, o.levels, c->pyr_scratch, c->pyr_scratch ? c->pyr_scratch + pyr : nullptr, d_mpyr,
                                        d_n_mask, d_start, d_part, d_work, d_arec, st));
    const MapStore one{nullptr, reinterpret_cast<MapEntry*>(d_in + up.entry), nullptr, 1, m};                   // (no state: the decide reads the entries only)
    HIPCHK(c, launch_keyframe_localise_decide(nullptr, 1, d_rrec, d_arec, nullptr, one, o, reinterpret_cast<LocaliseRec*>(d_out), st));      // (level 0 leads [levels][1])
    HIPCHK(c, hipMemcpyAsync(h_out.data(), d_out, out_total, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    memcpy(out, h_out.data(), sizeof(LocaliseRec));
    if (out_template) memcpy(out_template, h_out.data() + sizeof(LocaliseRec), NPIX);
    if (out_cover) memcpy(out_cover, h_out.data() + sizeof(LocaliseRec) + NPIX, NPIX);
    return HNET_OK;
}

// once, after hnet_sessions_enable_keyframe_map: templates, covers, mask pyramids, tables and records for max_batch and pinned blocks of its own
int hnet_sessions_enable_keyframe_localise(hnet_sessions* s) {
    const char* who = "hnet_sessions_enable_keyframe_localise";
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    hnet_keyframes* k = s->kf;
    if (!k || !k->map) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": the keyframe map is not enabled (hnet_sessions_enable_keyframe_map)");
    if (k->localise) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": the keyframe localise is already enabled");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const size_t B = (size_t)c->cfg.max_batch;
    auto l = std::make_unique<KeyLocalise>();
    hipError_t e = l->mem.alloc(&l->d_in, 2 * B);
    if (e == hipSuccess) e = l->mem.alloc(&l->tab, B);
    if (e == hipSuccess) e = l->mem.alloc(&l->rrec, B);
    if (e == hipSuccess) e = l->mem.alloc(&l->tmpl, B * NPIX);
    if (e == hipSuccess) e = l->mem.alloc(&l->cover, B * NPIX);
    if (e == hipSuccess) e = l->mem.alloc(&l->mpyr, B * PYR_BYTES);
    if (e == hipSuccess) e = l->mem.alloc(&l->n_mask, B * N_MASK);
    if (e == hipSuccess) e = l->mem.alloc(&l->d_out, B);
    if (e == hipSuccess) e = l->mem.alloc_pinned(&l->pin_in, 2 * B);
    if (e == hipSuccess) e = l->mem.alloc_pinned(&l->pin_out, B);
    if (e != hipSuccess) return fail(c, HNET_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    k->localise = l.release();
    return HNET_OK;
}

// ONE upload {ids | curr ring slot}; {render setup, eligible, render, gather + start, mask pyramid + masked alignment, decide} inside the store's events, on
// the context's staging and the store's alignment scratch; ONE download of the records [n], one synchronisation
int hnet_sessions_keyframe_localise(hnet_sessions* s, int n, const int32_t* ids, const hnet_keyframe_localise_opts* opts, hnet_keyframe_localise* out) {
    const char* who = "hnet_sessions_keyframe_localise";
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    hnet_keyframes* k = s->kf;
    if (!k || !k->map || !k->localise)
        return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": the keyframe localise is not enabled (hnet_sessions_enable_keyframe_localise)");
    KeyLocalise* l = static_cast<KeyLocalise*>(k->localise);
    if (!opts || !out) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": opts / out");
    LocaliseOpts o;
    int rc = check_opts(c, opts, who, o);
    if (rc != HNET_OK) return rc;
    if ((rc = sessions_check_ids(s, n, ids)) != HNET_OK) return rc;
    if ((rc = check_listed(s, n, ids, who, true)) != HNET_OK) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const int B = c->cfg.max_batch;
    slot_table(s, n, ids, nullptr, l->pin_in);
    const int32_t *d_ids = l->d_in, *d_slot = l->d_in + n;
    const size_t pyr = (size_t)B * PYR_BYTES;
    if (o.levels > 1 && (rc = ensure_pyr_scratch(c)) != HNET_OK) return rc;
    uint8_t* curr = (uint8_t*)c->stage_curr;
    const MapStore& map = k->map->dev;
    const RenderSource src = render_source(k);
    const AlignScratch al = KeyScratch(k->scratch, B).align();
    const RenderOpts ro{IMG_W, IMG_H, o.mode, 0};
    RobustOpts ao;
    memcpy(&ao, &o.align, sizeof ao);
    hipStream_t st = c->stream;
    if ((rc = begin_call(c, k, l->d_in, l->pin_in, 2 * (size_t)n * sizeof(int32_t))) != HNET_OK) return rc;
    HIPCHK(c, launch_keyframe_render_setup(d_ids, n, src, nullptr, l->tab, l->rrec, st));
    HIPCHK(c, launch_keyframe_localise_eligible(d_ids, n, map, l->tab, l->rrec, st));
    HIPCHK(c, launch_keyframe_render(d_ids, n, src, l->tab, ro, l->tmpl, l->cover, l->rrec, st));
    HIPCHK(c, launch_keyframe_localise_gather(d_slot, n, s->ring, 2 * s->n, l->rrec, o, curr, al.x0, st));
    HIPCHK(c, launch_photo_align_masked(l->tmpl, l->cover, curr, n, al.x0, ao, o.levels, c->pyr_scratch, c->pyr_scratch ? c->pyr_scratch + pyr : nullptr, l->mpyr,
                                        l->n_mask, al.start, al.part, al.work, al.rec, st));
    HIPCHK(c, launch_keyframe_localise_decide(d_ids, n, l->rrec, al.rec, k->state, map, o, l->d_out, st));      // (level 0 leads [levels][n])
    return finish_call(c, k, l->d_out, l->pin_out, out, (size_t)n * sizeof(LocaliseRec));
}

}  // extern "C"
