// capi_photo_align.hip — the photometric alignment of include/hnet.h on host frames, in its two forms: hnet_photo_align_* / hnet_op_photo_align[_pyramid]
//  and hnet_photo_robust_* / hnet_op_photo_align_robust (gain / bias model and Huber weights), the latter also on the template pixels a mask
// admits (hnet_op_photo_align_masked).  The kernels and the launch sequence are kernels_photo_align.hip's and kernels_photo_masked.hip's.  The sessions forms (capi_sessions.hip) run on photo_align_run below.
#include "capi_internal.h"
#include "filters_refine_dev.h"
#include "photo_masked_dev.h"

using namespace hnet;
using namespace capi;

static_assert(sizeof(hnet_photo_align) == sizeof(AlignRec) && offsetof(hnet_photo_align, mse0) == offsetof(AlignRec, mse0) &&
              offsetof(hnet_photo_align, n_valid0) == offsetof(AlignRec, n_valid0) && offsetof(hnet_photo_align, lambda) == offsetof(AlignRec, lambda) &&
              offsetof(hnet_photo_align, info) == offsetof(AlignRec, info) && sizeof(hnet_photo_align_opts) == sizeof(AlignOpts) &&
              offsetof(hnet_photo_align_opts, lambda0) == offsetof(AlignOpts, lambda0), "hnet_photo_align / _opts are the layouts of include/hnet_photo_align.h");
static_assert((int)HNET_ALIGN_CONVERGED == hnet_align::CONVERGED && (int)HNET_ALIGN_SINGULAR == hnet_align::SINGULAR &&
              (int)HNET_ALIGN_DEGENERATE == hnet_align::DEGENERATE && (int)HNET_ALIGN_FEW_PIXELS == hnet_align::FEW_PIXELS &&
              (int)HNET_ALIGN_MAX_ITERATIONS == hnet_align::MAX_ITERATIONS && (int)HNET_ALIGN_MAX_LEVELS == hnet_align::MAX_LEVELS,
              "the flags of include/hnet_photo_align.h");
static_assert(sizeof(hnet_photo_robust) == sizeof(RobustRec) && offsetof(hnet_photo_robust, gain) == offsetof(RobustRec, gain) &&
              offsetof(hnet_photo_robust, n_outliers0) == offsetof(RobustRec, n_outliers0) && offsetof(hnet_photo_robust, grad10) == offsetof(RobustRec, grad10) &&
              offsetof(hnet_photo_robust, info10) == offsetof(RobustRec, info10) && sizeof(hnet_photo_robust_opts) == sizeof(RobustOpts) &&
              offsetof(hnet_photo_robust_opts, brightness) == offsetof(RobustOpts, brightness) && offsetof(hnet_photo_robust_opts, huber_k) == offsetof(RobustOpts, huber_k) &&
              offsetof(hnet_photo_robust_opts, bias0) == offsetof(RobustOpts, bias0), "hnet_photo_robust / _opts are the layouts of include/hnet_photo_robust.h");

namespace {

// The run of both forms on n pairs resident on the device: the scratch (n_start elements of start), the launch sequence between the ev_align events, ONE
// download and one synchronisation.  levels_out is transposed on the host: the device keeps the records [levels][n], a level's records being what its solve
// launches write.
// launch: (img1, img2, n, x0, const Opts&, levels, pyr1, pyr2, Start*, Sums*, Work*, Rec*, stream) -> hipError_t.
template <class Opts, class Start, class Sums, class Work, class Rec, class PubOpts, class PubRec, class Launch>
int run(hnet_ctx* c, const uint8_t* d_img1, const uint8_t* d_img2, int n, const float* d_x0, const PubOpts& opts, int levels, size_t n_start, const Launch& launch,
        PubRec* out, PubRec* levels_out) {
    static_assert(sizeof(Opts) == sizeof(PubOpts) && sizeof(Rec) == sizeof(PubRec), "the public layouts");
    Opts o;
    memcpy(&o, &opts, sizeof o);
    const size_t pyr = (size_t)c->cfg.max_batch * PYR_BYTES;
    if (levels > 1)
        if (const int rc = ensure_pyr_scratch(c); rc != HNET_OK) return rc;
    DevTemps t;
    Sums* d_part = nullptr;
    Work* d_work = nullptr;
    Rec* d_rec = nullptr;
    Start* d_start = nullptr;
    HIPCHK(c, t.alloc(&d_part, (size_t)n * PHOTO_SLICES));
    HIPCHK(c, t.alloc(&d_work, (size_t)n));
    HIPCHK(c, t.alloc(&d_rec, (size_t)n * levels));
    if (n_start) HIPCHK(c, t.alloc(&d_start, n_start));
    std::vector<Rec> h_rec((size_t)n * levels);
    HIPCHK(c, hipEventRecord(c->ev_align[0], c->stream));
    HIPCHK(c, launch(d_img1, d_img2, n, d_x0, o, levels, c->pyr_scratch, c->pyr_scratch ? c->pyr_scratch + pyr : nullptr, d_start, d_part, d_work, d_rec, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_align[1], c->stream));
    HIPCHK(c, hipMemcpyAsync(h_rec.data(), d_rec, h_rec.size() * sizeof(Rec), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev_align[0], c->ev_align[1]));
    c->photo_align_ms = ms;
    memcpy(out, h_rec.data(), (size_t)n * sizeof(Rec));
    if (levels_out)
        for (int i = 0; i < n; i++)
            for (int l = 0; l < levels; l++) memcpy(levels_out + (size_t)i * levels + l, &h_rec[(size_t)l * n + i], sizeof(Rec));
    return HNET_OK;
}

// alignment of n host frame pairs from offsets0_px: ONE upload {img1 | img2 | offsets}, the launch sequence of `levels` levels, ONE download, one synchronisation
template <class PubOpts, class PubRec>
int op_photo_align(hnet_ctx* c, const uint8_t* img1, const uint8_t* img2, int n, const float* offsets0_px, const PubOpts* opts,
                   int (*check_opts)(hnet_ctx*, const PubOpts*, const char*), int levels, PubRec* out, PubRec* levels_out, const char* who) {
    if (!c) return HNET_ERR_INVALID_ARG;
    if (!img1 || !img2 || !offsets0_px || !out || n < 1) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": frames / offsets / out, n >= 1");
    if (levels < 1 || levels > HNET_ALIGN_MAX_LEVELS) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": 1 <= levels <= 4");
    const int rc = check_opts(c, opts, who);
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
    return photo_align_run(c, d_in, d_in + img, n, reinterpret_cast<const float*>(d_in + 2 * img), *opts, levels, out, levels_out);
}

}  // namespace

namespace capi {

int photo_align_check_opts(hnet_ctx* c, const hnet_photo_align_opts* opts, const char* who) {
    AlignOpts o;
    if (opts) memcpy(&o, opts, sizeof o);
    if (!opts || !hnet_align::opts_valid(o))
        return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": opts: 0 <= max_iterations <= 32, min_valid >= 0, 0 < lambda0 <= 1e100, eps_px >= 0, all finite");
    return HNET_OK;
}

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

// the plain form needs a start array only below the coarsest level: levels = 1 is {accumulate, solve} pairs at d_x0 and nothing else
int photo_align_run(hnet_ctx* c, const uint8_t* d_img1, const uint8_t* d_img2, int n, const float* d_x0, const hnet_photo_align_opts& opts, int levels,
                    hnet_photo_align* out, hnet_photo_align* levels_out) {
    return run<AlignOpts, float, AlignSums, AlignWork, AlignRec>(c, d_img1, d_img2, n, d_x0, opts, levels, levels > 1 ? (size_t)n * 8 : 0, launch_photo_align_pyramid, out,
                                                                 levels_out);
}
int photo_align_run(hnet_ctx* c, const uint8_t* d_img1, const uint8_t* d_img2, int n, const float* d_x0, const hnet_photo_robust_opts& opts, int levels,
                    hnet_photo_robust* out, hnet_photo_robust* levels_out) {
    return run<RobustOpts, RobustStart, RobustSums, RobustWork, RobustRec>(c, d_img1, d_img2, n, d_x0, opts, levels, (size_t)n, launch_photo_align_robust, out, levels_out);
}
// the robust form on the template pixels d_mask1 admits: the mask pyramid and its counts are temporaries of the call
int photo_align_masked_run(hnet_ctx* c, const uint8_t* d_img1, const uint8_t* d_mask1, const uint8_t* d_img2, int n, const float* d_x0,
                           const hnet_photo_robust_opts& opts, int levels, hnet_photo_robust* out, hnet_photo_robust* levels_out) {
    DevTemps t;
    uint8_t* d_mpyr = nullptr;
    int32_t* d_n_mask = nullptr;
    HIPCHK(c, t.alloc(&d_mpyr, (size_t)n * PYR_BYTES));
    HIPCHK(c, t.alloc(&d_n_mask, (size_t)n * N_MASK));
    const auto launch = [=](const uint8_t* img1, const uint8_t* img2, int n_, const float* x0, const RobustOpts& o, int levels_, uint8_t* pyr1, uint8_t* pyr2,
                            RobustStart* start, RobustSums* part, RobustWork* work, RobustRec* rec, hipStream_t s) {
        return launch_photo_align_masked(img1, d_mask1, img2, n_, x0, o, levels_, pyr1, pyr2, d_mpyr, d_n_mask, start, part, work, rec, s);
    };
    return run<RobustOpts, RobustStart, RobustSums, RobustWork, RobustRec>(c, d_img1, d_img2, n, d_x0, opts, levels, (size_t)n, launch, out, levels_out);
}

}  // namespace capi

extern "C" {

void hnet_photo_align_default_opts(hnet_photo_align_opts* o) {
    if (!o) return;
    AlignOpts d;
    hnet_align::default_opts(d);
    memcpy(o, &d, sizeof d);
}

void hnet_photo_robust_default_opts(hnet_photo_robust_opts* o) {
    if (!o) return;
    RobustOpts d;
    hnet_robust::default_opts(d);
    memcpy(o, &d, sizeof d);
}

double hnet_last_photo_align_device_ms(hnet_ctx* c) { return c ? c->photo_align_ms : 0.0; }

int hnet_op_photo_align(hnet_ctx* c, const uint8_t* img1, const uint8_t* img2, int n, const float* offsets0_px, const hnet_photo_align_opts* opts, hnet_photo_align* out) {
    return op_photo_align(c, img1, img2, n, offsets0_px, opts, photo_align_check_opts, 1, out, (hnet_photo_align*)nullptr, "hnet_op_photo_align");
}

// the coarse-to-fine form: the pyramid launch and one launch sequence per level
int hnet_op_photo_align_pyramid(hnet_ctx* c, const uint8_t* img1, const uint8_t* img2, int n, const float* offsets0_px, const hnet_photo_align_opts* opts, int levels,
                                hnet_photo_align* out, hnet_photo_align* levels_out) {
    return op_photo_align(c, img1, img2, n, offsets0_px, opts, photo_align_check_opts, levels, out, levels_out, "hnet_op_photo_align_pyramid");
}

int hnet_op_photo_align_robust(hnet_ctx* c, const uint8_t* img1, const uint8_t* img2, int n, const float* offsets0_px, const hnet_photo_robust_opts* opts, int levels,
                               hnet_photo_robust* out, hnet_photo_robust* levels_out) {
    return op_photo_align(c, img1, img2, n, offsets0_px, opts, photo_robust_check_opts, levels, out, levels_out, "hnet_op_photo_align_robust");
}

// the same with a mask beside img1: ONE upload {img1 | mask1 | img2 | offsets}
int hnet_op_photo_align_masked(hnet_ctx* c, const uint8_t* img1, const uint8_t* mask1, const uint8_t* img2, int n, const float* offsets0_px,
                               const hnet_photo_robust_opts* opts, int levels, hnet_photo_robust* out, hnet_photo_robust* levels_out) {
    const char* who = "hnet_op_photo_align_masked";
    if (!c) return HNET_ERR_INVALID_ARG;
    if (!img1 || !mask1 || !img2 || !offsets0_px || !out || n < 1) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": frames / mask / offsets / out, n >= 1");
    if (levels < 1 || levels > HNET_ALIGN_MAX_LEVELS) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": 1 <= levels <= 4");
    const int rc = photo_robust_check_opts(c, opts, who);
    if (rc != HNET_OK) return rc;
    if (n > c->cfg.max_batch) return fail(c, HNET_ERR_CAPACITY, std::string(who) + ": n exceeds max_batch");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const size_t img = (size_t)n * NPIX, off_bytes = (size_t)n * 8 * sizeof(float), up = 3 * img + off_bytes;      // (NPIX is a multiple of 16: every section stays aligned)
    DevTemps t;
    uint8_t* d_in = nullptr;
    HIPCHK(c, t.alloc(&d_in, up));
    std::vector<uint8_t> h_in(up);
    memcpy(h_in.data(), img1, img);
    memcpy(h_in.data() + img, mask1, img);
    memcpy(h_in.data() + 2 * img, img2, img);
    memcpy(h_in.data() + 3 * img, offsets0_px, off_bytes);
    HIPCHK(c, hipMemcpyAsync(d_in, h_in.data(), up, hipMemcpyHostToDevice, c->stream));
    return photo_align_masked_run(c, d_in, d_in + img, d_in + 2 * img, n, reinterpret_cast<const float*>(d_in + 3 * img), *opts, levels, out, levels_out);
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
