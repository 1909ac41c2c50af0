// capi_keyframe_localise.hip — hnet_keyframe_localise_default_opts and hnet_op_keyframe_localise of include/hnet.h (keyframe_localise_dev.h,
// csrc/kernels_keyframe_localise.hip): a camera localised against its rendered keyframe map.  The operator-level call owns its buffers as
// device temporaries and runs the unchanged render (keyframe_render_dev.h) and the masked alignment (photo_masked_dev.h) between its two small kernels.
#include "sessions_internal.h"
#include "keyframe_localise_dev.h"

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

namespace capi {

// the localise of a store: sized at its enable for max_batch B
struct KeyLocalise {
    int32_t* d_in = nullptr;                   // device: a call's table {ids [n] | curr ring slot [n]}
    RenderTab* tab = nullptr;                  // device [B]
    RenderRec* rrec = nullptr;                 // device [B]
    uint8_t *tmpl = nullptr, *cover = nullptr; // device [B][NPIX] each: the templates and their cover images (the masks)
    uint8_t* mpyr = nullptr;                   // device [B][PYR_BYTES]
    int32_t* n_mask = nullptr;                 // device [B][N_MASK]
    LocaliseRec* d_out = nullptr;              // device [B]
    int32_t* pin_in = nullptr;                 // pinned: the table
    LocaliseRec* pin_out = nullptr;            // pinned: the records
    hipEvent_t ev[2] = {nullptr, nullptr};     // around the launch sequence of the last localise
};

void keyframes_localise_free(KeyLocalise* l) {
    if (!l) return;
    for (void* p : {(void*)l->d_in, (void*)l->tab, (void*)l->rrec, (void*)l->tmpl, (void*)l->cover, (void*)l->mpyr, (void*)l->n_mask, (void*)l->d_out})
        if (p) (void)hipFree(p);
    if (l->pin_in) (void)hipHostFree(l->pin_in);
    if (l->pin_out) (void)hipHostFree(l->pin_out);
    for (hipEvent_t e : l->ev)
        if (e) (void)hipEventDestroy(e);
    delete l;
}

}  // namespace capi

namespace {

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
    // the upload block: {id 0, padded to 8 bytes | view [9] f64 | entries [m] | images [m], 16-byte aligned | curr}
    const size_t view_off = 8, ent_off = view_off + 9 * sizeof(double), img_off = (ent_off + (size_t)m * sizeof(MapEntry) + 15) & ~(size_t)15;
    const size_t curr_off = img_off + (size_t)m * NPIX, in_total = curr_off + NPIX, out_total = sizeof(LocaliseRec) + 2 * (size_t)NPIX;
    std::vector<uint8_t> h_in(in_total, 0), h_out(out_total);
    memcpy(h_in.data() + view_off, h_origin_pred, 9 * sizeof(double));
    memcpy(h_in.data() + ent_off, entries, (size_t)m * sizeof(MapEntry));
    memcpy(h_in.data() + img_off, images, (size_t)m * NPIX);
    memcpy(h_in.data() + curr_off, curr, NPIX);
    const size_t pyr = (size_t)c->cfg.max_batch * PYR_BYTES;
    if (o.levels > 1 && !c->pyr_scratch) HIPCHK(c, dalloc(&c->pyr_scratch, 2 * pyr));
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
    HIPCHK(c, t.alloc(&d_in, in_total));
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
    const RenderSource src{d_in + img_off, reinterpret_cast<const MapEntry*>(d_in + ent_off), nullptr, 1, m};
    const int32_t* d_id = reinterpret_cast<const int32_t*>(d_in);
    const RenderOpts ro{IMG_W, IMG_H, o.mode, 0};
    RobustOpts ao;
    memcpy(&ao, &o.align, sizeof ao);
    uint8_t *d_tmpl = d_out + sizeof(LocaliseRec), *d_cover = d_tmpl + NPIX;
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(d_in, h_in.data(), in_total, hipMemcpyHostToDevice, st));
    HIPCHK(c, launch_keyframe_render_setup(d_id, 1, src, reinterpret_cast<const double*>(d_in + view_off), d_tab, d_rrec, st));
    HIPCHK(c, launch_keyframe_render(d_id, 1, src, d_tab, ro, d_tmpl, d_cover, d_rrec, st));
    HIPCHK(c, launch_keyframe_localise_start(d_rrec, 1, o, d_x0, st));
    HIPCHK(c, launch_photo_align_masked(d_tmpl, d_cover, d_in + curr_off, 1, d_x0, ao, o.levels, c->pyr_scratch, c->pyr_scratch ? c->pyr_scratch + pyr : nullptr, d_mpyr,
                                        d_n_mask, d_start, d_part, d_work, d_arec, st));
    const MapStore one{nullptr, const_cast<MapEntry*>(src.entry), nullptr, 1, m};                   // (no state: the decide reads the entries only)
    HIPCHK(c, launch_keyframe_localise_decide(nullptr, 1, d_rrec, d_arec, nullptr, one, o, reinterpret_cast<LocaliseRec*>(d_out), st));      // (level 0 leads [levels][1])
    HIPCHK(c, hipMemcpyAsync(h_out.data(), d_out, out_total, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    memcpy(out, h_out.data(), sizeof(LocaliseRec));
    if (out_template) memcpy(out_template, h_out.data() + sizeof(LocaliseRec), NPIX);
    if (out_cover) memcpy(out_cover, h_out.data() + sizeof(LocaliseRec) + NPIX, NPIX);
    return HNET_OK;
}

// once, after hnet_sessions_enable_keyframe_map: templates, covers, mask pyramids, tables and records for max_batch, pinned blocks and events of its own
int hnet_sessions_enable_keyframe_localise(hnet_sessions* s) {
    const char* who = "hnet_sessions_enable_keyframe_localise";
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    KeyLocaliseHooks hk;
    if (!keyframes_localise_hooks(s, &hk)) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": the keyframe map is not enabled (hnet_sessions_enable_keyframe_map)");
    if (*hk.localise) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": the keyframe localise is already enabled");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const size_t B = (size_t)c->cfg.max_batch;
    KeyLocalise* l = new KeyLocalise();
    hipError_t e = hipMalloc((void**)&l->d_in, 2 * B * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&l->tab, B * sizeof(RenderTab));
    if (e == hipSuccess) e = hipMalloc((void**)&l->rrec, B * sizeof(RenderRec));
    if (e == hipSuccess) e = hipMalloc((void**)&l->tmpl, B * NPIX);
    if (e == hipSuccess) e = hipMalloc((void**)&l->cover, B * NPIX);
    if (e == hipSuccess) e = hipMalloc((void**)&l->mpyr, B * PYR_BYTES);
    if (e == hipSuccess) e = hipMalloc((void**)&l->n_mask, B * N_MASK * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&l->d_out, B * sizeof(LocaliseRec));
    if (e == hipSuccess) e = hipHostMalloc((void**)&l->pin_in, 2 * B * sizeof(int32_t), hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void**)&l->pin_out, B * sizeof(LocaliseRec), hipHostMallocDefault);
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipEventCreate(&l->ev[i]);
    if (e != hipSuccess) {
        keyframes_localise_free(l);
        return fail(c, HNET_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    }
    *hk.localise = l;
    return HNET_OK;
}

// ONE upload {ids | curr ring slot}; {render setup, eligible, render, gather + start, mask pyramid + masked alignment, decide} inside the localise's own events, on
// the context's staging and the store's alignment scratch; ONE download of the records [n], one synchronisation
int hnet_sessions_keyframe_localise(hnet_sessions* s, int n, const int32_t* ids, const hnet_keyframe_localise_opts* opts, hnet_keyframe_localise* out) {
    const char* who = "hnet_sessions_keyframe_localise";
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    KeyLocaliseHooks hk;
    if (!keyframes_localise_hooks(s, &hk) || !*hk.localise)
        return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": the keyframe localise is not enabled (hnet_sessions_enable_keyframe_localise)");
    KeyLocalise* l = *hk.localise;
    if (!opts || !out) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": opts / out");
    LocaliseOpts o;
    int rc = check_opts(c, opts, who, o);
    if (rc != HNET_OK) return rc;
    if ((rc = sessions_check_ids(s, n, ids)) != HNET_OK) return rc;
    if ((rc = keyframes_check_tracked(s, n, ids, who)) != HNET_OK) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const int B = c->cfg.max_batch;
    for (int i = 0; i < n; i++) {
        l->pin_in[i] = ids[i];
        l->pin_in[n + i] = 2 * ids[i] + s->st[ids[i]].curr;
    }
    const int32_t *d_ids = l->d_in, *d_slot = l->d_in + n;
    const size_t pyr = (size_t)B * PYR_BYTES;
    if (o.levels > 1 && !c->pyr_scratch) HIPCHK(c, dalloc(&c->pyr_scratch, 2 * pyr));
    uint8_t* curr = (uint8_t*)c->stage_curr;
    const MapStore map{const_cast<uint8_t*>(hk.src.img), hk.entry, hk.mstate, hk.src.n_sessions, hk.src.capacity};
    const RenderOpts ro{IMG_W, IMG_H, o.mode, 0};
    RobustOpts ao;
    memcpy(&ao, &o.align, sizeof ao);
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(l->d_in, l->pin_in, 2 * (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipEventRecord(l->ev[0], st));
    HIPCHK(c, launch_keyframe_render_setup(d_ids, n, hk.src, nullptr, l->tab, l->rrec, st));
    HIPCHK(c, launch_keyframe_localise_eligible(d_ids, n, map, l->tab, l->rrec, st));
    HIPCHK(c, launch_keyframe_render(d_ids, n, hk.src, l->tab, ro, l->tmpl, l->cover, l->rrec, st));
    HIPCHK(c, launch_keyframe_localise_gather(d_slot, n, s->ring, 2 * s->n, l->rrec, o, curr, hk.align.x0, st));
    HIPCHK(c, launch_photo_align_masked(l->tmpl, l->cover, curr, n, hk.align.x0, ao, o.levels, c->pyr_scratch, c->pyr_scratch ? c->pyr_scratch + pyr : nullptr, l->mpyr,
                                        l->n_mask, hk.align.start, hk.align.part, hk.align.work, hk.align.rec, st));
    HIPCHK(c, launch_keyframe_localise_decide(d_ids, n, l->rrec, hk.align.rec, hk.state, map, o, l->d_out, st));      // (level 0 leads [levels][n])
    HIPCHK(c, hipEventRecord(l->ev[1], st));
    HIPCHK(c, hipMemcpyAsync(l->pin_out, l->d_out, (size_t)n * sizeof(LocaliseRec), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, l->ev[0], l->ev[1]));
    *hk.ms = ms;
    memcpy(out, l->pin_out, (size_t)n * sizeof(LocaliseRec));
    return HNET_OK;
}

}  // extern "C"
