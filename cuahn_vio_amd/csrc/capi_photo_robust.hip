// capi_photo_robust.hip — hnet_photo_robust_* and hnet_op_photo_align_robust of include/hnet.h (photo_robust_dev.h, csrc/kernels_photo_robust.hip):
// photometric alignment with a gain / bias model and Huber weights.  The sessions form (capi_sessions.hip) runs on photo_robust_run below.
#include "capi_internal.h"
#include "filters_refine_dev.h"

using namespace hnet;
using namespace capi;

static_assert(sizeof(hnet_photo_robust) == sizeof(RobustRec) && offsetof(hnet_photo_robust, gain) == offsetof(RobustRec, gain) &&
              offsetof(hnet_photo_robust, n_outliers0) == offsetof(RobustRec, n_outliers0) && offsetof(hnet_photo_robust, grad10) == offsetof(RobustRec, grad10) &&
              offsetof(hnet_photo_robust, info10) == offsetof(RobustRec, info10) && sizeof(hnet_photo_robust_opts) == sizeof(RobustOpts) &&
              offsetof(hnet_photo_robust_opts, brightness) == offsetof(RobustOpts, brightness) && offsetof(hnet_photo_robust_opts, huber_k) == offsetof(RobustOpts, huber_k) &&
              offsetof(hnet_photo_robust_opts, bias0) == offsetof(RobustOpts, bias0), "hnet_photo_robust / _opts are the layouts of include/hnet_photo_robust.h");

namespace capi {

int photo_robust_check_opts(hnet_ctx* c, const hnet_photo_robust_opts* opts, const char* who) {
    if (!opts) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": opts");
    const int rc = photo_align_check_opts(c, &opts->base, who);
    if (rc != HNET_OK) return rc;
    RobustOpts o;
    memcpy(&o, opts, sizeof o);
    if (!hnet_robust::opts_valid(o))
        return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": opts: brightness 0 / 1, huber_k >= 0, gain0 > 0, all finite; gain0 = 1 and bias0 = 0 with the model off");
    return HNET_OK;
}

// levels_out is transposed on the host: the device keeps the records [levels][n], a level's records being what its solve launches write
int photo_robust_run(hnet_ctx* c, const uint8_t* d_img1, const uint8_t* d_img2, int n, const float* d_x0, const hnet_photo_robust_opts& opts, int levels,
                     hnet_photo_robust* out, hnet_photo_robust* levels_out) {
    RobustOpts o;
    memcpy(&o, &opts, sizeof o);
    const size_t pyr = (size_t)c->cfg.max_batch * PYR_BYTES;
    if (levels > 1 && !c->pyr_scratch) HIPCHK(c, dalloc(&c->pyr_scratch, 2 * pyr));
    DevTemps t;
    RobustSums* d_part = nullptr;
    RobustWork* d_work = nullptr;
    RobustRec* d_rec = nullptr;
    RobustStart* d_start = nullptr;
    HIPCHK(c, t.alloc(&d_part, (size_t)n * PHOTO_SLICES));
    HIPCHK(c, t.alloc(&d_work, (size_t)n));
    HIPCHK(c, t.alloc(&d_rec, (size_t)n * levels));
    HIPCHK(c, t.alloc(&d_start, (size_t)n));
    std::vector<RobustRec> h_rec((size_t)n * levels);
    HIPCHK(c, hipEventRecord(c->ev_align[0], c->stream));
    HIPCHK(c, launch_photo_align_robust(d_img1, d_img2, n, d_x0, o, levels, c->pyr_scratch, c->pyr_scratch ? c->pyr_scratch + pyr : nullptr, d_start, d_part,
                                        d_work, d_rec, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_align[1], c->stream));
    HIPCHK(c, hipMemcpyAsync(h_rec.data(), d_rec, h_rec.size() * sizeof(RobustRec), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev_align[0], c->ev_align[1]));
    c->photo_align_ms = ms;
    memcpy(out, h_rec.data(), (size_t)n * sizeof(RobustRec));
    if (levels_out)
        for (int i = 0; i < n; i++)
            for (int l = 0; l < levels; l++) memcpy(levels_out + (size_t)i * levels + l, &h_rec[(size_t)l * n + i], sizeof(RobustRec));
    return HNET_OK;
}

}  // namespace capi

extern "C" {

void hnet_photo_robust_default_opts(hnet_photo_robust_opts* o) {
    if (!o) return;
    RobustOpts d;
    hnet_robust::default_opts(d);
    memcpy(o, &d, sizeof d);
}

// ONE upload {img1 | img2 | offsets}, the launch sequence of `levels` levels, ONE download, one synchronisation
int hnet_op_photo_align_robust(hnet_ctx* c, const uint8_t* img1, const uint8_t* img2, int n, const float* offsets0_px, const hnet_photo_robust_opts* opts, int levels,
                               hnet_photo_robust* out, hnet_photo_robust* levels_out) {
    const char* who = "hnet_op_photo_align_robust";
    if (!c) return HNET_ERR_INVALID_ARG;
    if (!img1 || !img2 || !offsets0_px || !out || n < 1) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": frames / offsets / out, n >= 1");
    if (levels < 1 || levels > HNET_ALIGN_MAX_LEVELS) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": 1 <= levels <= 4");
    const int rc = photo_robust_check_opts(c, opts, who);
    if (rc != HNET_OK) return rc;
    if (n > c->cfg.max_batch) return fail(c, HNET_ERR_CAPACITY, std::string(who) + ": n exceeds max_batch");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const size_t img = (size_t)n * NPIX, off_bytes = (size_t)n * 8 * sizeof(float), up = 2 * img + off_bytes;      // (NPIX is a multiple of 16: every section stays aligned)
    DevTemps t;
    uint8_t* d_in = nullptr;
    HIPCHK(c, t.alloc(&d_in, up));
    std::vector<uint8_t> h_in(up);
    memcpy(h_in.data(), img1, img);
    memcpy(h_in.data() + img, img2, img);
    memcpy(h_in.data() + 2 * img, offsets0_px, off_bytes);
    HIPCHK(c, hipMemcpyAsync(d_in, h_in.data(), up, hipMemcpyHostToDevice, c->stream));
    return photo_robust_run(c, d_in, d_in + img, n, reinterpret_cast<const float*>(d_in + 2 * img), *opts, levels, out, levels_out);
}

// the Schur complement of the brightness block: info8 = A_xx - A_xc A_cc^-1 A_cx, grad8 = g_x - A_xc A_cc^-1 g_c (include/hnet_photo_refine.h marginal)
int hnet_photo_robust_marginal(const hnet_photo_robust* rec, double info8[64], double grad8[8]) {
    if (!rec || !info8 || !grad8) return HNET_ERR_INVALID_ARG;
    RobustRec r;
    memcpy(&r, rec, sizeof r);
    if (!hnet_refine::marginal(r, info8, grad8)) return HNET_ERR_INVALID_ARG;
    return HNET_OK;
}

}  // extern "C"
