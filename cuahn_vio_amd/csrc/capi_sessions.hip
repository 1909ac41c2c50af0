// capi_sessions.hip — hnet_sessions_* of include/hnet.h: many camera streams on one context.  The object itself is defined in sessions_internal.h,
// which the filters on top of it (capi_filters.hip) read too.
#include "sessions_internal.h"

using namespace hnet;
using namespace capi;

namespace capi {

int sessions_check_ids(hnet_sessions* s, int n, const int32_t* ids) {
    hnet_ctx* c = s->ctx;
    if (!ids || n < 1) return fail(c, HNET_ERR_INVALID_ARG, "sessions: n < 1 or no ids");
    if (n > c->cfg.max_batch) return fail(c, HNET_ERR_CAPACITY, "sessions: n exceeds max_batch");
    int rc = HNET_OK;
    int i = 0;
    for (; i < n; i++) {
        if (ids[i] < 0 || ids[i] >= s->n) { rc = fail(c, HNET_ERR_INVALID_ARG, "sessions: id out of range"); break; }
        if (s->mark[ids[i]]) { rc = fail(c, HNET_ERR_INVALID_ARG, "sessions: id repeated in one call"); break; }
        s->mark[ids[i]] = 1;
    }
    for (int j = 0; j < i; j++) s->mark[ids[j]] = 0;
    return rc;
}

int sessions_check_pairs(hnet_sessions* s, int n, const int32_t* ids) {
    for (int i = 0; i < n; i++)
        if (s->st[ids[i]].count < 2) return fail(s->ctx, HNET_ERR_NOT_READY, "HNet cannot inference! Only has one image!");
    return HNET_OK;
}

}  // namespace capi

extern "C" {

static constexpr int HNET_SESSIONS_MAX = 1 << 16;
static size_t sessions_header(int n) { return ((size_t)n * 8 + 255) & ~(size_t)255; }      // slot + camera tables, 256-byte aligned frames behind them


// (on the context's device) pinned block of the next push with room for `bytes` (its previous upload has completed) and a device slab as large
static int sessions_stage(hnet_sessions* s, size_t bytes, uint8_t** pin) {
    hnet_ctx* c = s->ctx;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const int k = s->pin_next;
    HIPCHK(c, hipEventSynchronize(s->ev_pin[k]));
    if (s->pin_cap[k] < bytes) {
        if (s->pin[k]) HIPCHK(c, hipHostFree(s->pin[k]));
        s->pin[k] = nullptr;
        s->pin_cap[k] = 0;
        HIPCHK(c, hipHostMalloc((void**)&s->pin[k], bytes, hipHostMallocDefault));
        s->pin_cap[k] = bytes;
    }
    if (s->slab_cap < bytes) {
        HIPCHK(c, hipStreamSynchronize(c->stream));               // (earlier scatters may still read it)
        if (s->slab) HIPCHK(c, hipFree(s->slab));
        s->slab = nullptr;
        s->slab_cap = 0;
        HIPCHK(c, hipMalloc((void**)&s->slab, bytes));
        s->slab_cap = bytes;
    }
    *pin = s->pin[k];
    return HNET_OK;
}

// after a push was enqueued: the slot each session wrote, its count and time stamp (hnet_push_image, :134-148)
static int sessions_commit_push(hnet_sessions* s, int n, const int32_t* ids, const double* t) {
    hnet_ctx* c = s->ctx;
    HIPCHK(c, hipEventRecord(s->ev_pin[s->pin_next], c->stream));
    for (int i = 0; i < n; i++) {
        hnet_sessions::Sess& e = s->st[ids[i]];
        e.curr = e.count == 0 ? 0 : (e.curr ^ 1);
        e.count++;
        if (e.count >= 2 && t) e.t = t[i];
        e.t_push = t ? t[i] : NAN;
    }
    s->pin_next ^= 1;
    return HNET_OK;
}
static int sessions_slot(const hnet_sessions* s, int id) { const hnet_sessions::Sess& e = s->st[id]; return 2 * id + (e.count == 0 ? 0 : (e.curr ^ 1)); }

void hnet_destroy_sessions(hnet_sessions* s) {
    if (!s) return;
    hnet_ctx* c = s->ctx;
    (void)hipSetDevice(c->cfg.device_id);
    (void)hipStreamSynchronize(c->stream);
    keyframes_destroy(s);
    auto fr = [](void* p) { if (p) (void)hipFree(p); };
    fr(s->ring); fr(s->slab); fr(s->d_tab); fr((void*)s->d_maps);
    for (auto& k : s->cams) { fr(k.map[0]); fr(k.map[1]); }
    for (int i = 0; i < 2; i++) {
        if (s->pin[i]) (void)hipHostFree(s->pin[i]);
        if (s->ev_pin[i]) (void)hipEventDestroy(s->ev_pin[i]);
    }
    if (s->pin_tab) (void)hipHostFree(s->pin_tab);
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    delete s;
}

int hnet_create_sessions(hnet_ctx* c, int n_sessions, hnet_sessions** out) {
    if (!c || !out) return HNET_ERR_INVALID_ARG;
    if (n_sessions < 1 || n_sessions > HNET_SESSIONS_MAX) return fail(c, HNET_ERR_INVALID_ARG, "hnet_create_sessions: n_sessions outside 1 .. 65536");
    if (c->s_begin != 0 || c->n_local != c->cfg.mc_samples) return fail(c, HNET_ERR_UNSUPPORTED, "hnet_create_sessions: the context evaluates a sample shard");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    hnet_sessions* s = new hnet_sessions();
    s->ctx = c;
    s->n = n_sessions;
    s->st.resize(n_sessions);
    s->mark.assign(n_sessions, 0);
    const size_t tab = (size_t)c->cfg.max_batch * (8 + 32 + 8);
    hipError_t e = hipMalloc((void**)&s->ring, (size_t)n_sessions * 2 * NPIX);
    if (e == hipSuccess) e = hipHostMalloc((void**)&s->pin_tab, tab, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void**)&s->d_tab, tab);
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipEventCreateWithFlags(&s->ev_pin[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreate(&s->ev0);
    if (e == hipSuccess) e = hipEventCreate(&s->ev1);
    if (e != hipSuccess) {
        hnet_destroy_sessions(s);
        return fail(c, HNET_ERR_DEVICE, std::string("hnet_create_sessions: ") + hipGetErrorString(e));
    }
    *out = s;
    return HNET_OK;
}

int hnet_sessions_push(hnet_sessions* s, int n, const int32_t* ids, const uint8_t* frames, int row_stride, size_t frame_stride, const double* t) {
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    if (!frames || row_stride < IMG_W || (n > 1 && frame_stride < (size_t)(IMG_H - 1) * row_stride + IMG_W))
        return fail(c, HNET_ERR_INVALID_ARG, "hnet_sessions_push: frames must be 224x320 8-bit, row_stride >= 320, frames apart by frame_stride");
    int rc = sessions_check_ids(s, n, ids);
    if (rc != HNET_OK) return rc;
    const size_t hdr = sessions_header(n), bytes = hdr + (size_t)n * NPIX;
    uint8_t* pin = nullptr;
    if ((rc = sessions_stage(s, bytes, &pin)) != HNET_OK) return rc;
    int32_t* dst = reinterpret_cast<int32_t*>(pin);
    for (int i = 0; i < n; i++) {
        dst[i] = sessions_slot(s, ids[i]);
        const uint8_t* f = frames + (size_t)i * frame_stride;
        uint8_t* o = pin + hdr + (size_t)i * NPIX;
        if (row_stride == IMG_W) memcpy(o, f, NPIX);
        else for (int r = 0; r < IMG_H; r++) memcpy(o + (size_t)r * IMG_W, f + (size_t)r * row_stride, IMG_W);
    }
    HIPCHK(c, hipMemcpyAsync(s->slab, pin, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_session_scatter(s->slab + hdr, reinterpret_cast<const int32_t*>(s->slab), n, 2 * s->n, s->ring, c->stream));
    return sessions_commit_push(s, n, ids, t);
}

int hnet_sessions_add_camera(hnet_sessions* s, const hnet_camera* cam, int* cam_id) {
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    if (!cam || !cam_id || cam->raw_rows < 1 || cam->raw_cols < 1 || cam->raw_rows > 16384 || cam->raw_cols > 16384)
        return fail(c, HNET_ERR_INVALID_ARG, "hnet_sessions_add_camera: camera");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    std::vector<float> mx, my;
    build_undistort_maps(cam, mx, my);
    hnet_sessions::Cam k = {{nullptr, nullptr}, cam->raw_rows, cam->raw_cols};
    DevTemps tmp;                                                  // (freed unless the camera is committed below)
    HIPCHK(c, tmp.alloc(&k.map[0], (size_t)NPIX));
    HIPCHK(c, tmp.alloc(&k.map[1], (size_t)NPIX));
    HIPCHK(c, hipMemcpy(k.map[0], mx.data(), NPIX * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(k.map[1], my.data(), NPIX * 4, hipMemcpyHostToDevice));
    std::vector<const float*> tab;
    for (auto& q : s->cams) { tab.push_back(q.map[0]); tab.push_back(q.map[1]); }
    tab.push_back(k.map[0]);
    tab.push_back(k.map[1]);
    const float** d_maps = nullptr;
    HIPCHK(c, tmp.alloc(&d_maps, tab.size()));
    HIPCHK(c, hipMemcpy(d_maps, tab.data(), tab.size() * sizeof(float*), hipMemcpyHostToDevice));
    HIPCHK(c, hipStreamSynchronize(c->stream));                    // enqueued remaps read the old table
    tmp.ptrs.clear();
    if (s->d_maps) (void)hipFree((void*)s->d_maps);
    s->d_maps = d_maps;
    s->cams.push_back(k);
    *cam_id = (int)s->cams.size() - 1;
    return HNET_OK;
}

int hnet_sessions_bind_camera(hnet_sessions* s, int id, int cam_id) {
    if (!s) return HNET_ERR_INVALID_ARG;
    if (id < 0 || id >= s->n || cam_id < 0 || cam_id >= (int)s->cams.size()) return fail(s->ctx, HNET_ERR_INVALID_ARG, "hnet_sessions_bind_camera: id or camera");
    s->st[id].cam = cam_id;
    return HNET_OK;
}

int hnet_sessions_push_raw(hnet_sessions* s, int n, const int32_t* ids, const uint8_t* raw, int rows, int cols, int row_stride, size_t frame_stride,
                           const double* t) {
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    if (!raw || rows < 1 || cols < 1 || row_stride < cols || (n > 1 && frame_stride < (size_t)(rows - 1) * row_stride + cols))
        return fail(c, HNET_ERR_INVALID_ARG, "hnet_sessions_push_raw: raw frame geometry");
    int rc = sessions_check_ids(s, n, ids);
    if (rc != HNET_OK) return rc;
    for (int i = 0; i < n; i++) {
        const int k = s->st[ids[i]].cam;
        if (k < 0) return fail(c, HNET_ERR_INVALID_ARG, "hnet_sessions_push_raw: session without a camera (hnet_sessions_bind_camera)");
        if (s->cams[k].rows != rows || s->cams[k].cols != cols) return fail(c, HNET_ERR_INVALID_ARG, "hnet_sessions_push_raw: raw image size differs from the camera's");
    }
    const size_t frame = ((size_t)rows * cols + 15) & ~(size_t)15;
    const size_t hdr = sessions_header(n), bytes = hdr + (size_t)n * frame;
    uint8_t* pin = nullptr;
    if ((rc = sessions_stage(s, bytes, &pin)) != HNET_OK) return rc;
    int32_t* dst = reinterpret_cast<int32_t*>(pin);
    for (int i = 0; i < n; i++) {
        dst[i] = sessions_slot(s, ids[i]);
        dst[n + i] = s->st[ids[i]].cam;
        const uint8_t* f = raw + (size_t)i * frame_stride;
        uint8_t* o = pin + hdr + (size_t)i * frame;
        for (int r = 0; r < rows; r++) memcpy(o + (size_t)r * cols, f + (size_t)r * row_stride, cols);
    }
    HIPCHK(c, hipMemcpyAsync(s->slab, pin, bytes, hipMemcpyHostToDevice, c->stream));
    const int32_t* d_dst = reinterpret_cast<const int32_t*>(s->slab);
    HIPCHK(c, launch_session_remap(s->slab + hdr, frame, rows, cols, d_dst, d_dst + n, s->d_maps, (int)s->cams.size(), n, 2 * s->n, s->ring, c->stream));
    return sessions_commit_push(s, n, ids, t);
}

int hnet_sessions_set_iterative_model(hnet_sessions* s, hnet_ctx* it) {
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    if (it) {                                                      // (the adapter's require_prior_agrees; the forwards read the main context's staging)
        if (it == c) return fail(c, HNET_ERR_INVALID_ARG, "hnet_sessions_set_iterative_model: the sessions' own context");
        if (it->cfg.device_id != c->cfg.device_id) return fail(c, HNET_ERR_INVALID_ARG, "hnet_sessions_set_iterative_model: both contexts must live on one device");
        if (it->s_begin != 0 || it->n_local != it->cfg.mc_samples) return fail(c, HNET_ERR_UNSUPPORTED, "hnet_sessions_set_iterative_model: the context evaluates a sample shard");
        if (!it->cfg.use_prior != !c->cfg.use_prior) return fail(c, HNET_ERR_INVALID_ARG, "hnet_sessions_set_iterative_model: use_prior differs from the main model's");
        if (it->cfg.max_batch < c->cfg.max_batch) return fail(c, HNET_ERR_INVALID_ARG, "hnet_sessions_set_iterative_model: max_batch below the main context's");
    }
    s->iter = it;
    return HNET_OK;
}

int hnet_sessions_infer(hnet_sessions* s, int n, const int32_t* ids, const double* prior_px, float* mean, float* cov, uint8_t* err_map) {
    return hnet_sessions_infer_iter(s, 0, n, ids, prior_px, mean, cov, err_map);
}

int hnet_sessions_infer_iter(hnet_sessions* s, int iteration, int n, const int32_t* ids, const double* prior_px, float* mean, float* cov, uint8_t* err_map) {
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    if (!mean || !cov) return fail(c, HNET_ERR_INVALID_ARG, "hnet_sessions_infer: mean / cov");
    if (iteration < 0) return fail(c, HNET_ERR_INVALID_ARG, "hnet_sessions_infer_iter: iteration < 0");
    int rc = sessions_check_ids(s, n, ids);
    if (rc != HNET_OK) return rc;
    hnet_ctx* m = iteration > 0 && s->iter ? s->iter : c;         // the model that runs (HomographyNet.cpp:183, :211); its forward is enqueued on c's stream
    hnet_ctx* const ctx[2] = {c, m != c ? m : nullptr};
    if (err_map && !m->cfg.emit_error_map) return fail(c, HNET_ERR_INVALID_ARG, "context was created without emit_error_map");
    if (c->cfg.use_prior && !prior_px) return fail(c, HNET_ERR_INVALID_ARG, "prior required");
    if ((rc = sessions_check_pairs(s, n, ids)) != HNET_OK) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    auto t0 = std::chrono::steady_clock::now();
    // ONE pinned block, ONE upload: the sequence numbers, the priors (:160-165 toType(kFloat)) and the (prev, curr) ring slots of every pair
    float* pr = reinterpret_cast<float*>(s->pin_tab);
    uint64_t* seq = reinterpret_cast<uint64_t*>(pr + (size_t)8 * n);
    int32_t* pairs = reinterpret_cast<int32_t*>(seq + n);
    for (int i = 0; i < n; i++) {
        const hnet_sessions::Sess& e = s->st[ids[i]];
        seq[i] = e.seq;
        for (int k = 0; k < 8; k++) pr[8 * i + k] = c->cfg.use_prior ? (float)prior_px[8 * i + k] : 0.0f;
        sessions_pair(s, ids[i], pairs + 2 * i);
    }
    const size_t bytes = (size_t)n * (8 + 32 + 8);
    const float* d_pr = reinterpret_cast<const float*>(s->d_tab);
    const uint64_t* d_seq = reinterpret_cast<const uint64_t*>(d_pr + (size_t)8 * n);
    const int32_t* d_pairs = reinterpret_cast<const int32_t*>(d_seq + n);
    hipStream_t st = c->stream;
    // (the frame pair is gathered into c's staging whichever model reads it; an attached context's max_batch covers n)
    const FwdArgs a{.prev = c->stage_prev, .curr = c->stage_curr, .prior = c->cfg.use_prior ? d_pr : nullptr, .batch = n, .mean = m->d_mean, .cov = m->d_cov,
                    .err_u8 = err_map ? m->d_err_u8 : nullptr, .seq_tab = d_seq};
    auto enqueue = [&](uint32_t* flag_now) -> int {
        HIPCHK(c, hipMemcpyAsync(s->d_tab, s->pin_tab, bytes, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipEventRecord(s->ev0, st));
        HIPCHK(c, launch_session_gather(s->ring, 2 * s->n, d_pairs, n, (uint8_t*)c->stage_prev, (uint8_t*)c->stage_curr, st));
        const int r = forward(m, a, st);
        if (r != HNET_OK) return m == c ? r : fail(c, r, "iterative model: " + m->err);
        HIPCHK(c, hipEventRecord(s->ev1, st));
        HIPCHK(c, hipMemcpyAsync(mean, m->d_mean, (size_t)n * 8 * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(cov, m->d_cov, (size_t)n * 64 * sizeof(float), hipMemcpyDeviceToHost, st));
        if (err_map) HIPCHK(c, hipMemcpyAsync(err_map, m->d_err_u8, (size_t)n * NPIX, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(&flag_now[m == c ? 0 : 1], m->d_flag, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemsetAsync(m->d_flag, 0, 4, st));          // host results are inspected by run_host_call (as in hnet_infer_batch)
        HIPCHK(c, hipStreamSynchronize(st));
        return HNET_OK;
    };
    // a repeat reuses the same table: the counts advance once
    rc = run_host_call(ctx, enqueue, [&] {
        const bool o = !(all_finite(mean, (size_t)n * 8) && all_finite(cov, (size_t)n * 64)) && all_finite(c->cfg.use_prior ? prior_px : nullptr, (size_t)n * 8);
        return o ? (m == c ? 0 : 1) : -1;
    });
    if (rc != HNET_OK) return rc;
    for (int i = 0; i < n; i++) s->st[ids[i]].seq++;                  // n_inferences of each session's dedicated context (one count for both models)
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, s->ev0, s->ev1));
    record_timing(s->timing, ms, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), 1, iteration == 0);
    return HNET_OK;
}

int hnet_sessions_image_count(const hnet_sessions* s, int id) { return (s && id >= 0 && id < s->n) ? s->st[id].count : -1; }
double hnet_sessions_latest_time(const hnet_sessions* s, int id) { return (s && id >= 0 && id < s->n) ? s->st[id].t : -1.0; }
uint64_t hnet_sessions_seq(const hnet_sessions* s, int id) { return (s && id >= 0 && id < s->n) ? s->st[id].seq : 0; }

int hnet_sessions_set_seq(hnet_sessions* s, int id, uint64_t seq) {
    if (!s) return HNET_ERR_INVALID_ARG;
    if (id < 0 || id >= s->n) return fail(s->ctx, HNET_ERR_INVALID_ARG, "sessions: id out of range");
    s->st[id].seq = seq;
    return HNET_OK;
}

int hnet_sessions_reset(hnet_sessions* s, int id) {
    if (!s) return HNET_ERR_INVALID_ARG;
    if (id < 0 || id >= s->n) return fail(s->ctx, HNET_ERR_INVALID_ARG, "sessions: id out of range");
    s->st[id].count = 0;
    s->st[id].curr = 0;
    s->st[id].t = -1.0;
    s->st[id].t_push = NAN;
    return keyframes_drop(s, id);
}

int hnet_sessions_get_frame(hnet_sessions* s, int id, int which, uint8_t* out) {
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    if (!out || id < 0 || id >= s->n || (which != 0 && which != 1)) return fail(c, HNET_ERR_INVALID_ARG, "hnet_sessions_get_frame: id / which / out");
    const hnet_sessions::Sess& e = s->st[id];
    if (e.count < (which == 0 ? 2 : 1)) return fail(c, HNET_ERR_NOT_READY, "hnet_sessions_get_frame: no such frame yet");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipMemcpyAsync(out, s->ring + (size_t)(2 * id + (which == 1 ? e.curr : e.curr ^ 1)) * NPIX, NPIX, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HNET_OK;
}

int hnet_sessions_last_timing(const hnet_sessions* s, hnet_timing* out) {
    if (!s || !out) return HNET_ERR_INVALID_ARG;
    *out = s->timing;
    return HNET_OK;
}

// ---- photometric residual records (include/hnet.h): csrc/kernels_photo.hip on the sessions' current pairs (the filters' own records: capi_filters.hip) ----

int hnet_sessions_photo_residual(hnet_sessions* s, int n, const int32_t* ids, const float* offsets_px, int m, hnet_photo_residual* out) {
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    if (!offsets_px || !out || m < 1 || m > PHOTO_MAX_CAND) return fail(c, HNET_ERR_INVALID_ARG, "hnet_sessions_photo_residual: offsets / out, 1 <= m <= 66");
    int rc = sessions_check_ids(s, n, ids);
    if (rc == HNET_OK) rc = sessions_check_pairs(s, n, ids);
    if (rc != HNET_OK) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    // ONE upload {offsets [n][m][8] f32 | pair table [n][2] i32}; nothing of the sessions' own tables, events or bookkeeping is touched
    const size_t off_bytes = (size_t)n * m * 8 * sizeof(float), up = off_bytes + (size_t)n * 8, rec_bytes = (size_t)n * m * sizeof(PhotoRec);
    std::vector<uint8_t> h_in(up), h_out(rec_bytes);
    memcpy(h_in.data(), offsets_px, off_bytes);
    for (int i = 0; i < n; i++) sessions_pair(s, ids[i], reinterpret_cast<int32_t*>(h_in.data() + off_bytes) + 2 * i);
    DevTemps t;
    uint8_t* d_in = nullptr;
    PhotoRec *d_part = nullptr, *d_rec = nullptr;
    HIPCHK(c, t.alloc(&d_in, up));
    HIPCHK(c, t.alloc(&d_part, photo_partial_count(n, m)));
    HIPCHK(c, t.alloc(&d_rec, (size_t)n * m));
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(d_in, h_in.data(), up, hipMemcpyHostToDevice, st));
    HIPCHK(c, launch_session_gather(s->ring, 2 * s->n, reinterpret_cast<const int32_t*>(d_in + off_bytes), n, (uint8_t*)c->stage_prev, (uint8_t*)c->stage_curr, st));
    const PhotoCands cands{reinterpret_cast<const float*>(d_in), nullptr, nullptr, 0};
    HIPCHK(c, launch_photo_residual((const uint8_t*)c->stage_prev, (const uint8_t*)c->stage_curr, n, cands, m, d_part, d_rec, nullptr, st));
    HIPCHK(c, hipMemcpyAsync(h_out.data(), d_rec, rec_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    memcpy(out, h_out.data(), rec_bytes);
    return HNET_OK;
}

// ---- photometric alignment (include/hnet.h hnet_photo_align) on the sessions' current pairs; read-only like the records above ----

// the front of the plain and the gain / bias + Huber form: the checks, the upload, the gather of the pairs, then the form's run
extern "C++" {
template <class PubOpts, class PubRec>
static int sessions_photo_align(hnet_sessions* s, int n, const int32_t* ids, const float* offsets0_px, const PubOpts* opts,
                                int (*check_opts)(hnet_ctx*, const PubOpts*, const char*), int levels, PubRec* out, PubRec* levels_out, const char* who) {
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    if (!offsets0_px || !out) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": offsets / out");
    if (levels < 1 || levels > HNET_ALIGN_MAX_LEVELS) return fail(c, HNET_ERR_INVALID_ARG, std::string(who) + ": 1 <= levels <= 4");
    int rc = check_opts(c, opts, who);
    if (rc == HNET_OK) rc = sessions_check_ids(s, n, ids);
    if (rc == HNET_OK) rc = sessions_check_pairs(s, n, ids);
    if (rc != HNET_OK) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    // ONE upload {offsets [n][8] f32 | pair table [n][2] i32}; nothing of the sessions' own tables, events or bookkeeping is touched
    const size_t off_bytes = (size_t)n * 8 * sizeof(float), up = off_bytes + (size_t)n * 8;
    std::vector<uint8_t> h_in(up);
    memcpy(h_in.data(), offsets0_px, off_bytes);
    for (int i = 0; i < n; i++) sessions_pair(s, ids[i], reinterpret_cast<int32_t*>(h_in.data() + off_bytes) + 2 * i);
    DevTemps t;
    uint8_t* d_in = nullptr;
    HIPCHK(c, t.alloc(&d_in, up));
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(d_in, h_in.data(), up, hipMemcpyHostToDevice, st));
    HIPCHK(c, launch_session_gather(s->ring, 2 * s->n, reinterpret_cast<const int32_t*>(d_in + off_bytes), n, (uint8_t*)c->stage_prev, (uint8_t*)c->stage_curr, st));
    return photo_align_run(c, (const uint8_t*)c->stage_prev, (const uint8_t*)c->stage_curr, n, reinterpret_cast<const float*>(d_in), *opts, levels, out, levels_out);
}
}  // extern "C++"

int hnet_sessions_photo_align(hnet_sessions* s, int n, const int32_t* ids, const float* offsets0_px, const hnet_photo_align_opts* opts, hnet_photo_align* out) {
    return sessions_photo_align(s, n, ids, offsets0_px, opts, photo_align_check_opts, 1, out, (hnet_photo_align*)nullptr, "hnet_sessions_photo_align");
}

// the coarse-to-fine form on the sessions' current pairs; read-only in the same way
int hnet_sessions_photo_align_pyramid(hnet_sessions* s, int n, const int32_t* ids, const float* offsets0_px, const hnet_photo_align_opts* opts, int levels,
                                      hnet_photo_align* out, hnet_photo_align* levels_out) {
    return sessions_photo_align(s, n, ids, offsets0_px, opts, photo_align_check_opts, levels, out, levels_out, "hnet_sessions_photo_align_pyramid");
}

// the gain / bias + Huber form on the sessions' current pairs; read-only in the same way, the same upload and gather
int hnet_sessions_photo_align_robust(hnet_sessions* s, int n, const int32_t* ids, const float* offsets0_px, const hnet_photo_robust_opts* opts, int levels,
                                     hnet_photo_robust* out, hnet_photo_robust* levels_out) {
    return sessions_photo_align(s, n, ids, offsets0_px, opts, photo_robust_check_opts, levels, out, levels_out, "hnet_sessions_photo_align_robust");
}

}  // extern "C"
