// capi_sessions.hip — hnet_sessions_* (many camera streams on one context) and hnet_filters_* (one device filter per session) of include/hnet.h.
#include "capi_internal.h"

using namespace hnet;
using namespace capi;

extern "C" {

// ---- sessions: many camera streams on one context (include/hnet.h).  Per session: image count, ring orientation, time stamp, mask sequence number and camera, all
// on the host; the frames live in a device ring of 2 slots per session (slot 2 id + k).  Every device step runs on the context's stream.
struct hnet_sessions {
    hnet_ctx* ctx = nullptr;
    hnet_ctx* iter = nullptr;                  // the iterative model's context (hnet_sessions_set_iterative_model) or null: forwards of iteration > 0, on ctx's stream
    int n = 0;
    uint8_t* ring = nullptr;                   // device [n][2][NPIX]
    // t_push: the stamp of the latest push, whatever the count (NaN: none given; hnet_filters_advance's t_frame)
    struct Sess { int count = 0, curr = 0, cam = -1; double t = -1.0; uint64_t seq = 0; double t_push = NAN; };
    std::vector<Sess> st;
    std::vector<uint8_t> mark;                 // id validation scratch (repeats within one call)
    struct Cam { float* map[2]; int rows, cols; };
    std::vector<Cam> cams;
    const float** d_maps = nullptr;            // device [cams][2]: the map pointers session_remap_kernel reads
    // push: two pinned blocks used in turn (the ev_img pattern of hnet_push_image), each {slot table [n] i32, camera table [n] i32 | frames}, and one device slab
    uint8_t* pin[2] = {nullptr, nullptr};
    size_t pin_cap[2] = {0, 0};
    hipEvent_t ev_pin[2] = {nullptr, nullptr};
    int pin_next = 0;
    uint8_t* slab = nullptr;
    size_t slab_cap = 0;
    // infer: ONE pinned block {priors [n][8] f32 | seq table [n] u64 | pair table [n][2] i32} and its device copy, sized for max_batch
    uint8_t* pin_tab = nullptr;
    uint8_t* d_tab = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hnet_timing timing = {};
};

static constexpr int HNET_SESSIONS_MAX = 1 << 16;
static size_t sessions_header(int n) { return ((size_t)n * 8 + 255) & ~(size_t)255; }      // slot + camera tables, 256-byte aligned frames behind them

// n distinct ids in range, n within the context's capacity
static int sessions_check_ids(hnet_sessions* s, int n, const int32_t* ids) {
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
// the (prev, curr) ring slots of session `id`'s pair, as launch_session_gather reads them
static void sessions_pair(const hnet_sessions* s, int id, int32_t* pair) { pair[0] = 2 * id + (s->st[id].curr ^ 1); pair[1] = 2 * id + s->st[id].curr; }

void hnet_destroy_sessions(hnet_sessions* s) {
    if (!s) return;
    hnet_ctx* c = s->ctx;
    (void)hipSetDevice(c->cfg.device_id);
    (void)hipStreamSynchronize(c->stream);
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
    for (int i = 0; i < n; i++)
        if (s->st[ids[i]].count < 2) return fail(c, HNET_ERR_NOT_READY, "HNet cannot inference! Only has one image!");   // :155-158, per session
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
    return HNET_OK;
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

// ---- filters: one 27-state filter per session of a sessions object (include/hnet.h).  Device: the states [n_sessions], the parameters [n_sessions] and
// the step's buffers sized for max_batch; host: each state's time (the t_frame check) and camera-IMU offset (the selection window).  A step works on a
// copy of the listed states (work) and scatters it back only once its forwards are accepted: an overflow / timeout repeat starts from the untouched states.
struct hnet_filters {
    hnet_sessions* s = nullptr;
    int iters = 1;
    FilterRec* d_state = nullptr;              // [n_sessions]
    FilterParams* d_params = nullptr;          // [n_sessions]
    std::vector<double> t, cam_imu_dt;         // host mirror of state t / the offset of each session
    std::vector<int> imu_avg;
    // step outputs, ONE device block {net [iters][B][72] f32 | prior_px [iters][B][8] f32 | updates [B] i32 | work [B] FilterRec} and its pinned copy
    uint8_t* d_out = nullptr;
    uint8_t* pin_out = nullptr;
    size_t off_prior = 0, off_upd = 0, off_work = 0, out_bytes = 0;
    double* d_prior_cam = nullptr;             // [B][8]
    // step inputs, ONE pinned block and its device copy (grown on demand): {readings [R] | t_frame [n] | seq [iters][n] | ids [n] | gate [n] | pairs [n][2] | rd_off [n + 1]}
    uint8_t* pin_in = nullptr;
    uint8_t* d_in = nullptr;
    size_t in_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hnet_timing timing = {};
    int last_n = 0;                            // sessions of the last accepted step (hnet_filters_last_priors)
    // ---- the IMU feed (hnet_filters_enable_feed): per session a device ring of `cap` readings, its head / count mirrored here, the newest reading's time,
    // whether the filter has a state (set_state or the initialiser) and, while it has none, the stamp of the last frame the initialiser dropped
    int cap = 0;
    hnet_ekf::ImuData* d_ring = nullptr;       // [n_sessions][cap]
    ImuRingMeta* d_meta = nullptr;             // [n_sessions]
    InitParams* d_ip = nullptr;                // [n_sessions]
    hnet_ekf::ImuData* d_sel = nullptr;        // [B][2 (cap + 2)]: filter_select_kernel's span and selection
    std::vector<ImuRingMeta> meta;
    std::vector<double> imu_newest, t_seen;
    std::vector<uint8_t> inited;
    std::vector<hnet_init_params> ip;
    std::vector<int> last_slot;                // session -> its workgroup in the last advance, -1 if none (hnet_filters_last_selection)
    // feed_imu: ONE pinned block {segments [n] | readings} and its device copy (grown on demand); ev_feed: the pinned block's last upload
    uint8_t* pin_feed = nullptr;
    uint8_t* d_feed = nullptr;
    size_t feed_cap = 0;
    hipEvent_t ev_feed = nullptr;
    // advance: ONE pinned block {jobs [B] | seq [iters][B] | gate [B] | ids [B] | pairs [B][2]} and its device copy; the results [B] behind the step's output block
    uint8_t* pin_adv = nullptr;
    uint8_t* d_adv = nullptr;
    size_t off_res = 0;
    // predict (hnet_filters_predict), allocated by its first call: ONE block {jobs [B] | records [B]}, its pinned copy, and the kernel's own scratch
    uint8_t* pin_pred = nullptr;
    uint8_t* d_pred = nullptr;
    hnet_ekf::ImuData* d_pred_sel = nullptr;   // [B][2 (cap + 2)]
    size_t off_pred_out = 0;
    hipEvent_t ev_p0 = nullptr, ev_p1 = nullptr;
    bool pred_timed = false;                   // set by the first hnet_filters_last_predict_device_ms: only then a predict records its two events
    double pred_ms = NAN;
    // innovations (hnet_filters_enable_innovations): the output block then is {net | prior_px | updates | innov [iters][n] InnovRec, dense | work | results},
    // so that the records lie inside the one download; the per-session gates; the statistics, accumulated from the records of accepted steps
    bool innov = false;
    size_t off_innov = 0;
    double* d_max_nis = nullptr;               // [n_sessions], 0 = no gate
    std::vector<hnet_innovation_stats> innov_stats;
    int last_innov_n = 0;                      // sessions the last accepted step has records for; 0: it ran with innovations off
    // photometric residual records (hnet_filters_enable_photometric): the output block then also holds {photo [n][2 + iters] PhotoRec, dense} behind the
    // innovation records (if any), inside the one download; the slice partials of kernels_photo.hip are device scratch
    bool photo = false;
    size_t off_photo = 0;
    PhotoRec* d_photo_part = nullptr;          // [B][2 + iters][PHOTO_SLICES]
    int last_photo_n = 0;                      // as last_innov_n
};

static size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// the offsets of the step's output block for max_batch B: {net | prior_px | updates | innov (if enabled) | photo (if enabled) | work | results}
static void filters_out_layout(hnet_filters* f, int B, bool innov, bool photo) {
    f->off_prior = al256((size_t)f->iters * B * 72 * sizeof(float));
    f->off_upd = f->off_prior + al256((size_t)f->iters * B * 8 * sizeof(float));
    f->off_innov = f->off_upd + al256((size_t)B * sizeof(int32_t));
    f->off_photo = f->off_innov + (innov ? al256((size_t)f->iters * B * sizeof(InnovRec)) : 0);
    f->off_work = f->off_photo + (photo ? al256((size_t)(2 + f->iters) * B * sizeof(PhotoRec)) : 0);
    f->off_res = f->off_work + al256((size_t)B * sizeof(FilterRec));
    f->out_bytes = f->off_res + (size_t)B * sizeof(AdvanceResult);
}
// what a step of n stepping sessions downloads in one copy from the start of the output block when the states are not wanted: up to the last record section in use
static size_t filters_down_head(const hnet_filters* f, int n) {
    if (f->photo) return f->off_photo + (size_t)n * (2 + f->iters) * sizeof(PhotoRec);
    if (f->innov) return f->off_innov + (size_t)f->iters * n * sizeof(InnovRec);
    return f->off_upd + (size_t)n * sizeof(int32_t);
}
// (photometric enabled) the records of the step's n pairs in the context's staging: candidates zero | prior of iteration 0 | packed mean of every forward
static hipError_t filters_launch_photo(hnet_filters* f, int n, hipStream_t st) {
    hnet_ctx* c = f->s->ctx;
    const PhotoCands cands{nullptr, reinterpret_cast<const float*>(f->d_out + f->off_prior), reinterpret_cast<const float*>(f->d_out), (size_t)c->cfg.max_batch * 72};
    return launch_photo_residual((const uint8_t*)c->stage_prev, (const uint8_t*)c->stage_curr, n, cands, 2 + f->iters, f->d_photo_part,
                                 reinterpret_cast<PhotoRec*>(f->d_out + f->off_photo), nullptr, st);
}
// after an accepted step with innovations on: the records [iters][n] of the sessions ids[0 .. n) go into their statistics
static void filters_count_innovations(hnet_filters* f, int n, const int32_t* ids) {
    const InnovRec* rec = reinterpret_cast<const InnovRec*>(f->pin_out + f->off_innov);
    for (int it = 0; it < f->iters; it++)
        for (int j = 0; j < n; j++) {
            const InnovRec& r = rec[(size_t)it * n + j];
            hnet_innovation_stats& a = f->innov_stats[ids[j]];
            if (r.flag == HNET_INNOV_USED) { a.used++; a.sum_nis += r.nis; }
            else if (r.flag == HNET_INNOV_REJECTED) a.rejected++;
            else if (r.flag == HNET_INNOV_SINGULAR) a.singular++;
            if ((r.flag == HNET_INNOV_USED || r.flag == HNET_INNOV_REJECTED) && r.nis > a.max_nis) a.max_nis = r.nis;
        }
}

// the context of forwards 1 .. iters - 1 of a step when the sessions have an iterative model (hnet_sessions_set_iterative_model), else null
static hnet_ctx* filters_iter_ctx(const hnet_filters* f) { return f->iters > 1 ? f->s->iter : nullptr; }
// forward `it` of a step: 0 on the main context ctx[0], later ones on ctx[1] if there is one; both read the pairs gathered into ctx[0]'s staging
static int filters_forward(hnet_ctx* const ctx[2], int it, const FwdArgs& a, hipStream_t st) {
    hnet_ctx* m = it > 0 && ctx[1] ? ctx[1] : ctx[0];
    const int r = forward(m, a, st);
    return r == HNET_OK || m == ctx[0] ? r : fail(ctx[0], r, "iterative model: " + m->err);
}
// the end of a step's attempt: the flag word of every context that ran downloaded and cleared (run_host_call), the one synchronisation
static int filters_flags(hnet_ctx* const ctx[2], uint32_t* flag, hipStream_t st) {
    hnet_ctx* c = ctx[0];
    for (int k = 0; k < 2; k++)
        if (ctx[k]) {
            HIPCHK(c, hipMemcpyAsync(&flag[k], ctx[k]->d_flag, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipMemsetAsync(ctx[k]->d_flag, 0, 4, st));
        }
    HIPCHK(c, hipStreamSynchronize(st));
    return HNET_OK;
}

void hnet_filter_default_params(hnet_filter_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    static const double T[12] = {-0.027256691772188965, -0.9996260641688061, 0.0021919370477445077, 0.02422852666805565,
                                 -0.7139206120417471, 0.017931469899155242, -0.6999970157716363, 0.008974432843748055,
                                 0.6996959571525168, -0.020644471939022302, -0.714142404092339, -0.000638971731537894};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) p->c_R_i[i * 3 + j] = T[i * 4 + j];
    for (int i = 0; i < 3; i++) p->i_t_i2c[i] = -(p->c_R_i[i] * T[3] + p->c_R_i[3 + i] * T[7] + p->c_R_i[6 + i] * T[11]);
    p->sigma_w = 0.00559017;
    p->sigma_wb = 8.94427e-04;
    p->sigma_a = 0.01118034;
    p->sigma_ab = 0.04472136;
    p->gravity_mag = 9.81;
    p->k_net_cov = 10.0;
    p->cam_imu_dt = 0.0;
    p->imu_avg = 1;
}

static FilterParams filter_params_dev(const hnet_filter_params& p) {
    FilterParams d;
    memset(&d, 0, sizeof d);
    memcpy(d.ext.c_R_i, p.c_R_i, sizeof d.ext.c_R_i);
    memcpy(d.ext.i_t_i2c, p.i_t_i2c, sizeof d.ext.i_t_i2c);
    hnet_ekf::noise_q_diag(p.sigma_w, p.sigma_a, p.sigma_wb, p.sigma_ab, d.q);
    d.gravity_mag = p.gravity_mag;
    d.k_net_cov = p.k_net_cov;
    d.imu_avg = p.imu_avg ? 1 : 0;
    return d;
}

void hnet_destroy_filters(hnet_filters* f) {
    if (!f) return;
    hnet_ctx* c = f->s->ctx;
    (void)hipSetDevice(c->cfg.device_id);
    (void)hipStreamSynchronize(c->stream);
    auto fr = [](void* p) { if (p) (void)hipFree(p); };
    fr(f->d_state); fr(f->d_params); fr(f->d_out); fr(f->d_prior_cam); fr(f->d_in);
    fr(f->d_ring); fr(f->d_meta); fr(f->d_ip); fr(f->d_sel); fr(f->d_feed); fr(f->d_adv); fr(f->d_pred); fr(f->d_pred_sel); fr(f->d_max_nis); fr(f->d_photo_part);
    if (f->pin_pred) (void)hipHostFree(f->pin_pred);
    if (f->ev_p0) (void)hipEventDestroy(f->ev_p0);
    if (f->ev_p1) (void)hipEventDestroy(f->ev_p1);
    if (f->pin_feed) (void)hipHostFree(f->pin_feed);
    if (f->pin_adv) (void)hipHostFree(f->pin_adv);
    if (f->ev_feed) (void)hipEventDestroy(f->ev_feed);
    if (f->pin_out) (void)hipHostFree(f->pin_out);
    if (f->pin_in) (void)hipHostFree(f->pin_in);
    if (f->ev0) (void)hipEventDestroy(f->ev0);
    if (f->ev1) (void)hipEventDestroy(f->ev1);
    delete f;
}

int hnet_create_filters(hnet_sessions* s, int max_iekf_iteration, hnet_filters** out) {
    if (!s || !out) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    if (max_iekf_iteration < 1 || max_iekf_iteration > 64) return fail(c, HNET_ERR_INVALID_ARG, "hnet_create_filters: max_iekf_iteration outside 1 .. 64");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    hnet_filters* f = new hnet_filters();
    f->s = s;
    f->iters = max_iekf_iteration;
    const int N = s->n, B = c->cfg.max_batch;
    hnet_filter_params dp;
    hnet_filter_default_params(&dp);
    f->t.assign(N, 0.0);
    f->cam_imu_dt.assign(N, dp.cam_imu_dt);
    f->imu_avg.assign(N, dp.imu_avg);
    filters_out_layout(f, B, false, false);
    f->t_seen.assign(N, -INFINITY);
    f->inited.assign(N, 0);
    f->last_slot.assign(N, -1);
    hnet_init_params ip0;
    hnet_filter_default_init_params(&ip0);
    f->ip.assign(N, ip0);
    std::vector<FilterRec> st(N);
    memset(st.data(), 0, st.size() * sizeof(FilterRec));
    for (auto& r : st) r.s.q[0] = 1.0;
    std::vector<FilterParams> pr(N, filter_params_dev(dp));
    hipError_t e = hipMalloc((void**)&f->d_state, (size_t)N * sizeof(FilterRec));
    if (e == hipSuccess) e = hipMalloc((void**)&f->d_params, (size_t)N * sizeof(FilterParams));
    if (e == hipSuccess) e = hipMalloc((void**)&f->d_out, f->out_bytes);
    if (e == hipSuccess) e = hipHostMalloc((void**)&f->pin_out, f->out_bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void**)&f->d_prior_cam, (size_t)B * 8 * sizeof(double));
    if (e == hipSuccess) e = hipEventCreate(&f->ev0);
    if (e == hipSuccess) e = hipEventCreate(&f->ev1);
    if (e == hipSuccess) e = hipMemcpyAsync(f->d_state, st.data(), (size_t)N * sizeof(FilterRec), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(f->d_params, pr.data(), (size_t)N * sizeof(FilterParams), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        hnet_destroy_filters(f);
        return fail(c, HNET_ERR_DEVICE, std::string("hnet_create_filters: ") + hipGetErrorString(e));
    }
    *out = f;
    return HNET_OK;
}

int hnet_filters_set_params(hnet_filters* f, int id, const hnet_filter_params* p) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = f->s->ctx;
    if (!p || id < 0 || id >= f->s->n) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_set_params: id or params");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const FilterParams d = filter_params_dev(*p);
    HIPCHK(c, hipMemcpyAsync(f->d_params + id, &d, sizeof d, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    f->cam_imu_dt[id] = p->cam_imu_dt;
    f->imu_avg[id] = p->imu_avg ? 1 : 0;
    return HNET_OK;
}

static_assert(sizeof(hnet_filter_state) == sizeof(FilterRec), "hnet_filter_state is the FilterRec layout");

int hnet_filters_set_state(hnet_filters* f, int id, const hnet_filter_state* st) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = f->s->ctx;
    if (!st || id < 0 || id >= f->s->n) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_set_state: id or state");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipMemcpyAsync(f->d_state + id, st, sizeof(FilterRec), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    f->t[id] = st->t;
    f->inited[id] = 1;
    return HNET_OK;
}

int hnet_filters_get_state(hnet_filters* f, int n, const int32_t* ids, hnet_filter_state* out) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = f->s->ctx;
    if (!ids || !out || n < 1) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_get_state: ids / out");
    for (int i = 0; i < n; i++)
        if (ids[i] < 0 || ids[i] >= f->s->n) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_get_state: id out of range");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    for (int i = 0; i < n; i++) HIPCHK(c, hipMemcpyAsync(out + i, f->d_state + ids[i], sizeof(FilterRec), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HNET_OK;
}

int hnet_filters_step(hnet_filters* f, int n, const int32_t* ids, const double* t_frame, const hnet_imu* imu, const int64_t* imu_off,
                      hnet_filter_state* state_out, float* net_out, int32_t* updates) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_sessions* s = f->s;
    hnet_ctx* c = s->ctx;
    if (!t_frame || !imu_off) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_step: t_frame / imu_off");
    int rc = sessions_check_ids(s, n, ids);
    if (rc != HNET_OK) return rc;
    for (int i = 0; i < n; i++)
        if (s->st[ids[i]].count < 2) return fail(c, HNET_ERR_NOT_READY, "HNet cannot inference! Only has one image!");
    for (int i = 0; i < n; i++) {
        if (!(t_frame[i] > f->t[ids[i]]) || !std::isfinite(t_frame[i]))
            return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_step: t_frame must be later than the state's time (Propagator.cpp:32-43)");
        if (imu_off[i] < 0 || imu_off[i + 1] < imu_off[i] || (imu_off[i + 1] > imu_off[i] && !imu))
            return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_step: imu / imu_off");
    }
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    auto t0 = std::chrono::steady_clock::now();
    const int I = f->iters;
    // selection on the host (hnet_ekf::select_imu_readings: the window [state t, t_frame] + the session's offset) into the input block
    static_assert(sizeof(hnet_imu) == sizeof(hnet_ekf::ImuData), "hnet_imu is hnet_ekf::ImuData");
    int64_t total = 0;
    for (int i = 0; i < n; i++) total += imu_off[i + 1] - imu_off[i] + 2;
    const size_t o_t = al256((size_t)total * sizeof(hnet_ekf::ImuData)), o_seq = o_t + al256((size_t)n * 8), o_ids = o_seq + al256((size_t)I * n * 8);
    const size_t o_gate = o_ids + al256((size_t)n * 4), o_pairs = o_gate + al256((size_t)n * 4), o_off = o_pairs + al256((size_t)n * 8);
    const size_t in_bytes = o_off + al256((size_t)(n + 1) * 4);
    if (f->in_cap < in_bytes) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (f->pin_in) HIPCHK(c, hipHostFree(f->pin_in));
        if (f->d_in) HIPCHK(c, hipFree(f->d_in));
        f->pin_in = f->d_in = nullptr;
        f->in_cap = 0;
        HIPCHK(c, hipHostMalloc((void**)&f->pin_in, in_bytes, hipHostMallocDefault));
        HIPCHK(c, hipMalloc((void**)&f->d_in, in_bytes));
        f->in_cap = in_bytes;
    }
    hnet_ekf::ImuData* rd = reinterpret_cast<hnet_ekf::ImuData*>(f->pin_in);
    double* tf = reinterpret_cast<double*>(f->pin_in + o_t);
    uint64_t* seq = reinterpret_cast<uint64_t*>(f->pin_in + o_seq);
    int32_t* hid = reinterpret_cast<int32_t*>(f->pin_in + o_ids);
    int32_t* gate = reinterpret_cast<int32_t*>(f->pin_in + o_gate);
    int32_t* pairs = reinterpret_cast<int32_t*>(f->pin_in + o_pairs);
    int32_t* roff = reinterpret_cast<int32_t*>(f->pin_in + o_off);
    int R = 0;
    for (int i = 0; i < n; i++) {
        const int id = ids[i];
        const hnet_sessions::Sess& e = s->st[id];
        const int64_t m = imu_off[i + 1] - imu_off[i];
        const double dt = f->cam_imu_dt[id];
        roff[i] = R;
        R += hnet_ekf::select_imu_readings(reinterpret_cast<const hnet_ekf::ImuData*>(imu) + imu_off[i], (int)m, f->t[id] + dt, t_frame[i] + dt, rd + R);
        tf[i] = t_frame[i];
        for (int it = 0; it < I; it++) seq[(size_t)it * n + i] = e.seq + (uint64_t)it;
        hid[i] = id;
        gate[i] = (e.t == t_frame[i] && e.count > 10) ? 1 : 0;                      // VioManager.cpp:257
        sessions_pair(s, id, pairs + 2 * i);
    }
    roff[n] = R;
    const hnet_ekf::ImuData* d_rd = reinterpret_cast<const hnet_ekf::ImuData*>(f->d_in);
    const double* d_tf = reinterpret_cast<const double*>(f->d_in + o_t);
    const uint64_t* d_seq = reinterpret_cast<const uint64_t*>(f->d_in + o_seq);
    const int32_t* d_ids = reinterpret_cast<const int32_t*>(f->d_in + o_ids);
    int32_t* d_gate = reinterpret_cast<int32_t*>(f->d_in + o_gate);             // (filter_innovation_kernel closes the gate of a session it rejects; every attempt uploads it again)
    const int32_t* d_pairs = reinterpret_cast<const int32_t*>(f->d_in + o_pairs);
    const int32_t* d_roff = reinterpret_cast<const int32_t*>(f->d_in + o_off);
    float* d_net = reinterpret_cast<float*>(f->d_out);
    float* d_prior = reinterpret_cast<float*>(f->d_out + f->off_prior);
    int32_t* d_upd = reinterpret_cast<int32_t*>(f->d_out + f->off_upd);
    FilterRec* d_work = reinterpret_cast<FilterRec*>(f->d_out + f->off_work);
    const float* h_net = reinterpret_cast<const float*>(f->pin_out);
    const float* h_prior = reinterpret_cast<const float*>(f->pin_out + f->off_prior);
    // the output block is laid out for max_batch: download the used parts of each section in one copy up to the last one needed
    const size_t down = state_out ? f->off_work + (size_t)n * sizeof(FilterRec) : filters_down_head(f, n);
    InnovRec* d_innov = reinterpret_cast<InnovRec*>(f->d_out + f->off_innov);
    hipStream_t st = c->stream;
    const size_t up = o_off + (size_t)(n + 1) * 4;
    hnet_ctx* const ctx[2] = {c, filters_iter_ctx(f)};
    auto enqueue = [&](uint32_t* flag_now) -> int {
        HIPCHK(c, hipMemcpyAsync(f->d_in, f->pin_in, up, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemsetAsync(d_upd, 0, (size_t)n * sizeof(int32_t), st));
        HIPCHK(c, hipEventRecord(f->ev0, st));
        HIPCHK(c, launch_session_gather(s->ring, 2 * s->n, d_pairs, n, (uint8_t*)c->stage_prev, (uint8_t*)c->stage_curr, st));
        HIPCHK(c, launch_filter_propagate(d_ids, n, s->n, f->d_state, f->d_params, d_rd, d_roff, d_tf, d_work, st));
        for (int it = 0; it < I; it++) {
            float* pr_it = d_prior + (size_t)it * c->cfg.max_batch * 8;
            float* net_it = d_net + (size_t)it * c->cfg.max_batch * 72;
            HIPCHK(c, launch_filter_prior(d_work, n, pr_it, f->d_prior_cam, st));
            const FwdArgs a{.prev = c->stage_prev, .curr = c->stage_curr, .prior = c->cfg.use_prior ? pr_it : nullptr, .batch = n, .mean = net_it, .cov = net_it + 8,
                            .seq_tab = d_seq + (size_t)it * n, .mean_stride = HNET_PACKED_FLOATS, .cov_stride = HNET_PACKED_FLOATS};
            if (const int r = filters_forward(ctx, it, a, st); r != HNET_OK) return r;
            if (f->innov) HIPCHK(c, launch_filter_innovation(d_ids, n, s->n, f->d_params, d_work, net_it, f->d_prior_cam, f->d_max_nis, d_gate, d_upd, it, d_innov, st));
            HIPCHK(c, launch_filter_update(d_ids, n, s->n, f->d_params, net_it, f->d_prior_cam, d_gate, it != I - 1, it == I - 1, d_work, d_upd, st));
        }
        HIPCHK(c, hipEventRecord(f->ev1, st));
        if (f->photo) HIPCHK(c, filters_launch_photo(f, n, st));   // (behind ev1: hnet_filters_last_timing keeps its meaning; inside the attempt: a repeat recomputes the records)
        HIPCHK(c, hipMemcpyAsync(f->pin_out, f->d_out, down, hipMemcpyDeviceToHost, st));
        return filters_flags(ctx, flag_now, st);
    };
    // an overflow of the fp16 planes: the first forward with a non-finite output had finite inputs (its fp32 priors; later priors follow from it)
    auto overflowed = [&]() -> int {
        for (int it = 0; it < I; it++)
            if (!all_finite(h_net + (size_t)it * c->cfg.max_batch * 72, (size_t)n * 72))
                return !c->cfg.use_prior || all_finite(h_prior + (size_t)it * c->cfg.max_batch * 8, (size_t)n * 8) ? (it > 0 && ctx[1] ? 1 : 0) : -1;
        return -1;
    };
    if ((rc = run_host_call(ctx, enqueue, overflowed)) != HNET_OK) return rc;
    // accepted: the listed states take the step's result (stream order: later calls see it), the bookkeeping advances
    HIPCHK(c, launch_filter_scatter(d_work, d_ids, n, s->n, f->d_state, st));
    for (int i = 0; i < n; i++) {
        f->t[ids[i]] = t_frame[i];
        s->st[ids[i]].seq += (uint64_t)I;
    }
    if (net_out)
        for (int it = 0; it < I; it++) memcpy(net_out + (size_t)it * n * 72, h_net + (size_t)it * c->cfg.max_batch * 72, (size_t)n * 72 * sizeof(float));
    if (updates) memcpy(updates, f->pin_out + f->off_upd, (size_t)n * sizeof(int32_t));
    if (state_out) memcpy(state_out, f->pin_out + f->off_work, (size_t)n * sizeof(FilterRec));
    f->last_n = n;
    f->last_innov_n = f->innov ? n : 0;
    f->last_photo_n = f->photo ? n : 0;
    if (f->innov) filters_count_innovations(f, n, ids);
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, f->ev0, f->ev1));
    record_timing(f->timing, ms, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), I, true);
    return HNET_OK;
}

int hnet_filters_last_priors(const hnet_filters* f, int n, float* out) {
    if (!f || !out) return HNET_ERR_INVALID_ARG;
    if (f->last_n < 1) return fail(f->s->ctx, HNET_ERR_NOT_READY, "hnet_filters_last_priors: no step yet");
    if (n != f->last_n) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_last_priors: n differs from the last step's");
    const int B = f->s->ctx->cfg.max_batch;
    const float* h_prior = reinterpret_cast<const float*>(f->pin_out + f->off_prior);
    for (int it = 0; it < f->iters; it++) memcpy(out + (size_t)it * f->last_n * 8, h_prior + (size_t)it * B * 8, (size_t)f->last_n * 8 * sizeof(float));
    return HNET_OK;
}

int hnet_filters_last_timing(const hnet_filters* f, hnet_timing* out) {
    if (!f || !out) return HNET_ERR_INVALID_ARG;
    *out = f->timing;
    return HNET_OK;
}

// ---- filters, fed (include/hnet.h): the IMU rings, the initialiser and hnet_filters_advance ----

void hnet_filter_default_init_params(hnet_init_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->window_time = 1.0;
    p->imu_thresh = 0.5;
    p->init_height = 0.1;
    p->wait_for_jerk = 1;
}

static InitParams init_params_dev(const hnet_init_params& p) { return InitParams{p.window_time, p.imu_thresh, p.init_height, p.wait_for_jerk ? 1 : 0, 0}; }
// the advance input block for n sessions: jobs | seq [iters][n] | gate | ids | pairs
struct AdvLayout {
    size_t o_seq, o_gate, o_ids, o_pairs, bytes;
    AdvLayout(int n, int iters) {
        o_seq = al256((size_t)n * sizeof(AdvanceJob));
        o_gate = o_seq + al256((size_t)iters * n * 8);
        o_ids = o_gate + al256((size_t)n * 4);
        o_pairs = o_ids + al256((size_t)n * 4);
        bytes = o_pairs + al256((size_t)n * 8);
    }
};

int hnet_filters_enable_feed(hnet_filters* f, int imu_capacity) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = f->s->ctx;
    if (f->cap) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_enable_feed: already enabled");
    if (imu_capacity < 2 || imu_capacity > (1 << 20)) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_enable_feed: imu_capacity outside 2 .. 1048576");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const int N = f->s->n, B = c->cfg.max_batch;
    const size_t adv = AdvLayout(B, f->iters).bytes;
    std::vector<InitParams> ipd(N);
    for (int i = 0; i < N; i++) ipd[i] = init_params_dev(f->ip[i]);
    hipError_t e = hipMalloc((void**)&f->d_ring, (size_t)N * imu_capacity * sizeof(hnet_ekf::ImuData));
    if (e == hipSuccess) e = hipMalloc((void**)&f->d_meta, (size_t)N * sizeof(ImuRingMeta));
    if (e == hipSuccess) e = hipMalloc((void**)&f->d_ip, (size_t)N * sizeof(InitParams));
    if (e == hipSuccess) e = hipMalloc((void**)&f->d_sel, (size_t)B * 2 * (imu_capacity + 2) * sizeof(hnet_ekf::ImuData));
    if (e == hipSuccess) e = hipMalloc((void**)&f->d_adv, adv);
    if (e == hipSuccess) e = hipHostMalloc((void**)&f->pin_adv, adv, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&f->ev_feed, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMemsetAsync(f->d_meta, 0, (size_t)N * sizeof(ImuRingMeta), c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(f->d_ip, ipd.data(), (size_t)N * sizeof(InitParams), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        auto fr = [](void* q) { if (q) (void)hipFree(q); };
        fr(f->d_ring); fr(f->d_meta); fr(f->d_ip); fr(f->d_sel); fr(f->d_adv);
        if (f->pin_adv) (void)hipHostFree(f->pin_adv);
        if (f->ev_feed) (void)hipEventDestroy(f->ev_feed);
        f->d_ring = nullptr; f->d_meta = nullptr; f->d_ip = nullptr; f->d_sel = nullptr; f->d_adv = nullptr; f->pin_adv = nullptr; f->ev_feed = nullptr;
        return fail(c, HNET_ERR_DEVICE, std::string("hnet_filters_enable_feed: ") + hipGetErrorString(e));
    }
    f->meta.assign(N, ImuRingMeta{0, 0});
    f->imu_newest.assign(N, -INFINITY);
    f->cap = imu_capacity;
    return HNET_OK;
}

int hnet_filters_set_init_params(hnet_filters* f, int id, const hnet_init_params* p) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = f->s->ctx;
    if (!p || id < 0 || id >= f->s->n || !(p->window_time > 0.0) || !std::isfinite(p->window_time) || !std::isfinite(p->imu_thresh) || !std::isfinite(p->init_height))
        return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_set_init_params: id or params");
    if (f->cap) {
        HIPCHK(c, hipSetDevice(c->cfg.device_id));
        const InitParams d = init_params_dev(*p);
        HIPCHK(c, hipMemcpyAsync(f->d_ip + id, &d, sizeof d, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    f->ip[id] = *p;
    return HNET_OK;
}

int hnet_filters_feed_imu(hnet_filters* f, int n, const int32_t* ids, const hnet_imu* imu, const int64_t* imu_off) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_sessions* s = f->s;
    hnet_ctx* c = s->ctx;
    if (!f->cap) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_feed_imu: feed not enabled (hnet_filters_enable_feed)");
    if (!ids || !imu_off || n < 1 || n > s->n) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_feed_imu: ids / imu_off / n");
    if (imu_off[0] < 0) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_feed_imu: imu_off");
    // validation first: nothing is appended unless every listed session's readings are in order
    int rc = HNET_OK, marked = 0;
    for (int i = 0; i < n && rc == HNET_OK; i++) {
        const int id = ids[i];
        if (id < 0 || id >= s->n) { rc = fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_feed_imu: id out of range"); break; }
        if (s->mark[id]) { rc = fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_feed_imu: id repeated in one call"); break; }
        s->mark[id] = 1;
        marked = i + 1;
        if (imu_off[i + 1] < imu_off[i] || imu_off[i + 1] > INT32_MAX || (imu_off[i + 1] > imu_off[i] && !imu)) { rc = fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_feed_imu: imu / imu_off"); break; }
        double last = f->imu_newest[id];
        for (int64_t k = imu_off[i]; k < imu_off[i + 1]; k++) {
            if (!std::isfinite(imu[k].t) || imu[k].t < last) { rc = fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_feed_imu: readings must be finite and in non-decreasing time"); break; }
            last = imu[k].t;
        }
    }
    for (int j = 0; j < marked; j++) s->mark[ids[j]] = 0;
    if (rc != HNET_OK) return rc;
    const int64_t base = imu_off[0], total = imu_off[n] - base;
    if (total == 0) return HNET_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const size_t o_rd = al256((size_t)n * sizeof(ImuFeedSeg)), bytes = o_rd + (size_t)total * sizeof(hnet_ekf::ImuData);
    HIPCHK(c, hipEventSynchronize(f->ev_feed));                    // the pinned block's last upload has left it
    if (f->feed_cap < bytes) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (f->pin_feed) HIPCHK(c, hipHostFree(f->pin_feed));
        if (f->d_feed) HIPCHK(c, hipFree(f->d_feed));
        f->pin_feed = f->d_feed = nullptr;
        f->feed_cap = 0;
        const size_t want = std::max(bytes, (size_t)1 << 16);
        HIPCHK(c, hipHostMalloc((void**)&f->pin_feed, want, hipHostMallocDefault));
        HIPCHK(c, hipMalloc((void**)&f->d_feed, want));
        f->feed_cap = want;
    }
    static_assert(sizeof(hnet_imu) == sizeof(hnet_ekf::ImuData), "hnet_imu is hnet_ekf::ImuData");
    ImuFeedSeg* seg = reinterpret_cast<ImuFeedSeg*>(f->pin_feed);
    memcpy(f->pin_feed + o_rd, imu + base, (size_t)total * sizeof(hnet_imu));
    std::vector<ImuRingMeta> next(n);
    int longest = 0;
    for (int i = 0; i < n; i++) {
        const ImuRingMeta m = f->meta[ids[i]];
        const int64_t have = imu_off[i + 1] - imu_off[i];
        const int take = (int)std::min<int64_t>(have, f->cap);      // more than a ring's worth: only the newest `cap` can stay
        const int count = std::min(f->cap, m.count + take);
        const int head = (int)(((int64_t)m.head + m.count + take - count) % f->cap);
        next[i] = ImuRingMeta{head, count};
        seg[i] = ImuFeedSeg{ids[i], (int32_t)(imu_off[i] - base + (have - take)), take, (int32_t)(((int64_t)m.head + m.count) % f->cap), head, count};
        longest = std::max(longest, take);
    }
    HIPCHK(c, hipMemcpyAsync(f->d_feed, f->pin_feed, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(f->ev_feed, c->stream));
    HIPCHK(c, launch_imu_append(reinterpret_cast<const ImuFeedSeg*>(f->d_feed), n, longest, reinterpret_cast<const hnet_ekf::ImuData*>(f->d_feed + o_rd), (int)total,
                                s->n, f->cap, f->d_ring, f->d_meta, c->stream));
    for (int i = 0; i < n; i++) {
        f->meta[ids[i]] = next[i];
        if (imu_off[i + 1] > imu_off[i]) f->imu_newest[ids[i]] = imu[imu_off[i + 1] - 1].t;
    }
    return HNET_OK;
}

int hnet_filters_initialized(const hnet_filters* f, int id) { return (f && id >= 0 && id < f->s->n) ? (int)f->inited[id] : -1; }

int hnet_filters_uninitialize(hnet_filters* f, int id) {
    if (!f) return HNET_ERR_INVALID_ARG;
    if (id < 0 || id >= f->s->n) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_uninitialize: id out of range");
    f->inited[id] = 0;
    f->t_seen[id] = -INFINITY;
    return hnet_sessions_reset(f->s, id);
}

int hnet_filters_advance(hnet_filters* f, int n, const int32_t* ids, hnet_filter_state* state_out, float* net_out, int32_t* updates, int32_t* status) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_sessions* s = f->s;
    hnet_ctx* c = s->ctx;
    if (!f->cap) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_advance: feed not enabled (hnet_filters_enable_feed)");
    if (!status) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_advance: status");
    int rc = sessions_check_ids(s, n, ids);
    if (rc != HNET_OK) return rc;
    auto t_begin = std::chrono::steady_clock::now();
    const int I = f->iters, B = c->cfg.max_batch;
    // what each listed session does (VioManager.cpp:122-162); the sessions that step come first on the device, the propagate-only ones behind them
    std::vector<int> order;                                        // listed index of workgroup j
    order.reserve(n);
    for (int pass = 0; pass < 2; pass++)
        for (int i = 0; i < n; i++) {
            const int id = ids[i];
            const hnet_sessions::Sess& e = s->st[id];
            int st;
            if (e.count < 1 || !(e.t_push > (f->inited[id] ? f->t[id] : f->t_seen[id]))) st = HNET_ADV_NO_FRAME;
            else if (!(e.t_push < f->imu_newest[id] - f->cam_imu_dt[id])) st = HNET_ADV_WAIT_IMU;
            else if (!f->inited[id]) st = HNET_ADV_WAIT_INIT;      // (INITIALIZED if the device's initialiser accepts)
            else st = e.count < 2 ? HNET_ADV_PROPAGATED : HNET_ADV_STEPPED;
            if (pass == 0) status[i] = st;
            if ((pass == 0 && st == HNET_ADV_STEPPED) || (pass == 1 && (st == HNET_ADV_PROPAGATED || st == HNET_ADV_WAIT_INIT))) order.push_back(i);
        }
    const int n_a = (int)order.size();
    int n_s = 0;
    for (int i = 0; i < n; i++) n_s += status[i] == HNET_ADV_STEPPED;
    if (net_out) memset(net_out, 0, (size_t)I * n * 72 * sizeof(float));
    if (updates) memset(updates, 0, (size_t)n * sizeof(int32_t));
    std::fill(f->last_slot.begin(), f->last_slot.end(), -1);
    f->last_photo_n = 0;                                           // (a call in which nothing steps has no photometric records, whatever the call before it left)
    if (n_a == 0) return HNET_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const AdvLayout L(n_a, I);
    AdvanceJob* job = reinterpret_cast<AdvanceJob*>(f->pin_adv);
    uint64_t* seq = reinterpret_cast<uint64_t*>(f->pin_adv + L.o_seq);
    int32_t* gate = reinterpret_cast<int32_t*>(f->pin_adv + L.o_gate);
    int32_t* hid = reinterpret_cast<int32_t*>(f->pin_adv + L.o_ids);
    int32_t* pairs = reinterpret_cast<int32_t*>(f->pin_adv + L.o_pairs);
    bool any_init = false;
    for (int j = 0; j < n_a; j++) {
        const int i = order[j], id = ids[i];
        const hnet_sessions::Sess& e = s->st[id];
        const bool init = status[i] == HNET_ADV_WAIT_INIT;
        any_init |= init;
        job[j] = AdvanceJob{e.t_push, f->cam_imu_dt[id], id, init ? 1 : 0, j >= n_s ? 1 : 0, 0};
        for (int it = 0; it < I; it++) seq[(size_t)it * n_a + j] = e.seq + (uint64_t)it;
        gate[j] = (j < n_s && e.t == e.t_push && e.count > 10) ? 1 : 0;             // VioManager.cpp:257
        hid[j] = id;
        sessions_pair(s, id, pairs + 2 * j);
    }
    const AdvanceJob* d_job = reinterpret_cast<const AdvanceJob*>(f->d_adv);
    const uint64_t* d_seq = reinterpret_cast<const uint64_t*>(f->d_adv + L.o_seq);
    int32_t* d_gate = reinterpret_cast<int32_t*>(f->d_adv + L.o_gate);          // (as in hnet_filters_step)
    const int32_t* d_ids = reinterpret_cast<const int32_t*>(f->d_adv + L.o_ids);
    const int32_t* d_pairs = reinterpret_cast<const int32_t*>(f->d_adv + L.o_pairs);
    float* d_net = reinterpret_cast<float*>(f->d_out);
    float* d_prior = reinterpret_cast<float*>(f->d_out + f->off_prior);
    int32_t* d_upd = reinterpret_cast<int32_t*>(f->d_out + f->off_upd);
    FilterRec* d_work = reinterpret_cast<FilterRec*>(f->d_out + f->off_work);
    AdvanceResult* d_res = reinterpret_cast<AdvanceResult*>(f->d_out + f->off_res);
    InnovRec* d_innov = reinterpret_cast<InnovRec*>(f->d_out + f->off_innov);
    const float* h_net = reinterpret_cast<const float*>(f->pin_out);
    const float* h_prior = reinterpret_cast<const float*>(f->pin_out + f->off_prior);
    const AdvanceResult* h_res = reinterpret_cast<const AdvanceResult*>(f->pin_out + f->off_res);
    hipStream_t st = c->stream;
    hnet_ctx* const ctx[2] = {c, n_s ? filters_iter_ctx(f) : nullptr};
    auto enqueue = [&](uint32_t* flag_now) -> int {
        HIPCHK(c, hipMemcpyAsync(f->d_adv, f->pin_adv, L.bytes, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemsetAsync(d_upd, 0, (size_t)n_a * sizeof(int32_t), st));
        HIPCHK(c, hipEventRecord(f->ev0, st));
        if (any_init)                                              // (the sessions without a state are among the propagate-only ones)
            HIPCHK(c, launch_filter_init(d_job + n_s, n_a - n_s, s->n, f->cap, f->d_ring, f->d_meta, f->d_ip, f->d_params, d_work + n_s, d_res + n_s, st));
        HIPCHK(c, launch_filter_select(d_job, n_a, s->n, f->cap, f->d_ring, f->d_meta, f->d_state, d_work, f->d_sel, d_res, st));
        if (n_s) HIPCHK(c, launch_session_gather(s->ring, 2 * s->n, d_pairs, n_s, (uint8_t*)c->stage_prev, (uint8_t*)c->stage_curr, st));
        HIPCHK(c, launch_filter_propagate_adv(d_job, n_a, s->n, f->cap, f->d_state, f->d_params, f->d_sel, d_res, d_work, st));
        for (int it = 0; it < I && n_s; it++) {
            float* pr_it = d_prior + (size_t)it * B * 8;
            float* net_it = d_net + (size_t)it * B * 72;
            HIPCHK(c, launch_filter_prior(d_work, n_s, pr_it, f->d_prior_cam, st));
            const FwdArgs a{.prev = c->stage_prev, .curr = c->stage_curr, .prior = c->cfg.use_prior ? pr_it : nullptr, .batch = n_s, .mean = net_it, .cov = net_it + 8,
                            .seq_tab = d_seq + (size_t)it * n_a, .mean_stride = HNET_PACKED_FLOATS, .cov_stride = HNET_PACKED_FLOATS};
            if (const int r = filters_forward(ctx, it, a, st); r != HNET_OK) return r;
            if (f->innov) HIPCHK(c, launch_filter_innovation(d_ids, n_s, s->n, f->d_params, d_work, net_it, f->d_prior_cam, f->d_max_nis, d_gate, d_upd, it, d_innov, st));
            HIPCHK(c, launch_filter_update(d_ids, n_s, s->n, f->d_params, net_it, f->d_prior_cam, d_gate, it != I - 1, it == I - 1, d_work, d_upd, st));
        }
        HIPCHK(c, hipEventRecord(f->ev1, st));
        if (f->photo && n_s) HIPCHK(c, filters_launch_photo(f, n_s, st));          // (as in hnet_filters_step)
        if (n_s) HIPCHK(c, hipMemcpyAsync(f->pin_out, f->d_out, filters_down_head(f, n_s), hipMemcpyDeviceToHost, st));
        if (state_out) HIPCHK(c, hipMemcpyAsync(f->pin_out + f->off_work, d_work, (size_t)n_a * sizeof(FilterRec), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(f->pin_out + f->off_res, d_res, (size_t)n_a * sizeof(AdvanceResult), hipMemcpyDeviceToHost, st));
        return filters_flags(ctx, flag_now, st);
    };
    auto overflowed = [&]() -> int {                               // as hnet_filters_step, over the sessions that step
        for (int it = 0; it < I && n_s; it++)
            if (!all_finite(h_net + (size_t)it * B * 72, (size_t)n_s * 72))
                return !c->cfg.use_prior || all_finite(h_prior + (size_t)it * B * 8, (size_t)n_s * 8) ? (it > 0 && ctx[1] ? 1 : 0) : -1;
        return -1;
    };
    if ((rc = run_host_call(ctx, enqueue, overflowed)) != HNET_OK) return rc;
    // accepted: the states take the results (not those the initialiser refused), the bookkeeping advances
    HIPCHK(c, launch_filter_scatter_ok(d_work, d_job, d_res, n_a, s->n, f->d_state, st));
    const int32_t* h_upd = reinterpret_cast<const int32_t*>(f->pin_out + f->off_upd);
    for (int j = 0; j < n_a; j++) {
        const int i = order[j], id = ids[i];
        hnet_sessions::Sess& e = s->st[id];
        f->last_slot[id] = j;
        if (status[i] == HNET_ADV_WAIT_INIT) {
            if (!h_res[j].ok) {                                    // the frame is dropped: the session starts over (VioManager.cpp:158-162)
                f->t_seen[id] = e.t_push;
                e.count = 0;
                e.curr = 0;
                e.t = -1.0;
                continue;
            }
            status[i] = HNET_ADV_INITIALIZED;
            f->inited[id] = 1;
            f->t[id] = h_res[j].time0 > e.t_push ? h_res[j].time0 : e.t_push;
            e.count = 1;                                           // this frame is the session's first image; its ring slot stays the current one
            e.t = -1.0;
        } else {
            f->t[id] = e.t_push;
            if (j < n_s) {
                e.seq += (uint64_t)I;
                if (updates) updates[i] = h_upd[j];
                if (net_out)
                    for (int it = 0; it < I; it++) memcpy(net_out + ((size_t)it * n + i) * 72, h_net + ((size_t)it * B + j) * 72, 72 * sizeof(float));
            }
        }
        if (state_out) memcpy(state_out + i, f->pin_out + f->off_work + (size_t)j * sizeof(FilterRec), sizeof(FilterRec));
    }
    f->last_n = n_s;
    f->last_innov_n = f->innov ? n_s : 0;
    f->last_photo_n = f->photo ? n_s : 0;
    if (f->innov && n_s) filters_count_innovations(f, n_s, hid);             // (the stepping sessions are the first n_s of the call's id table)
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, f->ev0, f->ev1));
    record_timing(f->timing, ms, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(), n_s ? I : 0, true);
    return HNET_OK;
}

int hnet_filters_last_selection(hnet_filters* f, int id, hnet_imu* out, int cap, int* count) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = f->s->ctx;
    if (!f->cap) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_last_selection: feed not enabled");
    if (!count || id < 0 || id >= f->s->n || cap < 0 || (cap > 0 && !out)) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_last_selection: id / out / count");
    *count = 0;
    const int j = f->last_slot[id];
    if (j < 0) return HNET_OK;
    const AdvanceResult* h_res = reinterpret_cast<const AdvanceResult*>(f->pin_out + f->off_res);
    const int m = h_res[j].ok ? h_res[j].n_sel : 0;
    if (m < 0 || m > f->cap + 2) return fail(c, HNET_ERR_DEVICE, "hnet_filters_last_selection: selection count out of range");
    *count = m;
    const int k = std::min(m, cap);
    if (k > 0) {
        HIPCHK(c, hipSetDevice(c->cfg.device_id));
        HIPCHK(c, hipMemcpyAsync(out, f->d_sel + (size_t)j * 2 * (f->cap + 2) + (f->cap + 2), (size_t)k * sizeof(hnet_imu), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return HNET_OK;
}

// ---- filters, innovation records (include/hnet.h): the records themselves come from filter_innovation_kernel inside hnet_filters_step / _advance ----

static_assert(sizeof(hnet_innovation) == sizeof(InnovRec), "hnet_innovation is the InnovRec layout");
static_assert((int)HNET_INNOV_NONE == (int)hnet_ekf::INNOV_NONE && (int)HNET_INNOV_USED == (int)hnet_ekf::INNOV_USED && (int)HNET_INNOV_REJECTED == (int)hnet_ekf::INNOV_REJECTED &&
              (int)HNET_INNOV_SINGULAR == (int)hnet_ekf::INNOV_SINGULAR && (int)HNET_INNOV_SKIPPED == (int)hnet_ekf::INNOV_SKIPPED, "HNET_INNOV_* are the header's flags");

int hnet_filters_enable_innovations(hnet_filters* f) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = f->s->ctx;
    if (f->innov) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_enable_innovations: already enabled");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipStreamSynchronize(c->stream));                    // (nothing enqueued reads the old output block any more)
    const int N = f->s->n, B = c->cfg.max_batch;
    // the output block with room for the records: a new block, and the old one freed only when everything is there
    filters_out_layout(f, B, true, f->photo);
    uint8_t *d_out = nullptr, *pin_out = nullptr;
    double* d_max = nullptr;
    hipError_t e = hipMalloc((void**)&d_out, f->out_bytes);
    if (e == hipSuccess) e = hipHostMalloc((void**)&pin_out, f->out_bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void**)&d_max, (size_t)N * sizeof(double));
    if (e == hipSuccess) e = hipMemsetAsync(d_max, 0, (size_t)N * sizeof(double), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        if (d_out) (void)hipFree(d_out);
        if (pin_out) (void)hipHostFree(pin_out);
        if (d_max) (void)hipFree(d_max);
        filters_out_layout(f, B, false, f->photo);
        return fail(c, HNET_ERR_DEVICE, std::string("hnet_filters_enable_innovations: ") + hipGetErrorString(e));
    }
    (void)hipFree(f->d_out);
    (void)hipHostFree(f->pin_out);
    f->d_out = d_out;
    f->pin_out = pin_out;
    f->d_max_nis = d_max;
    f->innov_stats.assign(N, hnet_innovation_stats{0, 0, 0, 0.0, 0.0});
    f->last_n = 0;                                                 // what last_priors / last_selection described went with the old block
    f->last_innov_n = 0;
    f->last_photo_n = 0;
    std::fill(f->last_slot.begin(), f->last_slot.end(), -1);
    f->innov = true;
    return HNET_OK;
}

int hnet_filters_set_nis_gate(hnet_filters* f, int id, double max_nis) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = f->s->ctx;
    if (!f->innov) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_set_nis_gate: innovations not enabled (hnet_filters_enable_innovations)");
    if (id < 0 || id >= f->s->n || !(max_nis >= 0.0)) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_set_nis_gate: id out of range, or max_nis negative or NaN");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipMemcpyAsync(f->d_max_nis + id, &max_nis, sizeof max_nis, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HNET_OK;
}

int hnet_filters_last_innovations(const hnet_filters* f, int n, hnet_innovation* out) {
    if (!f || !out) return HNET_ERR_INVALID_ARG;
    if (!f->innov || f->last_innov_n < 1) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_last_innovations: the last step ran without innovations");
    if (n != f->last_innov_n) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_last_innovations: n differs from the last step's");
    memcpy(out, f->pin_out + f->off_innov, (size_t)f->iters * n * sizeof(InnovRec));
    return HNET_OK;
}

int hnet_filters_innovation_stats(const hnet_filters* f, int id, hnet_innovation_stats* out) {
    if (!f || !out) return HNET_ERR_INVALID_ARG;
    if (!f->innov || id < 0 || id >= f->s->n) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_innovation_stats: innovations not enabled or id out of range");
    *out = f->innov_stats[id];
    return HNET_OK;
}

int hnet_filters_reset_innovation_stats(hnet_filters* f, int id) {
    if (!f) return HNET_ERR_INVALID_ARG;
    if (!f->innov || id < 0 || id >= f->s->n) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_reset_innovation_stats: innovations not enabled or id out of range");
    f->innov_stats[id] = hnet_innovation_stats{0, 0, 0, 0.0, 0.0};
    return HNET_OK;
}

// ---- photometric residual records (include/hnet.h): csrc/kernels_photo.hip on the sessions' current pairs and inside hnet_filters_step / _advance ----

int hnet_sessions_photo_residual(hnet_sessions* s, int n, const int32_t* ids, const float* offsets_px, int m, hnet_photo_residual* out) {
    if (!s) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = s->ctx;
    if (!offsets_px || !out || m < 1 || m > PHOTO_MAX_CAND) return fail(c, HNET_ERR_INVALID_ARG, "hnet_sessions_photo_residual: offsets / out, 1 <= m <= 66");
    int rc = sessions_check_ids(s, n, ids);
    if (rc != HNET_OK) return rc;
    for (int i = 0; i < n; i++)
        if (s->st[ids[i]].count < 2) return fail(c, HNET_ERR_NOT_READY, "HNet cannot inference! Only has one image!");
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

int hnet_filters_enable_photometric(hnet_filters* f) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_ctx* c = f->s->ctx;
    if (f->photo) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_enable_photometric: already enabled");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipStreamSynchronize(c->stream));                    // (nothing enqueued reads the old output block any more)
    const int B = c->cfg.max_batch;
    // as hnet_filters_enable_innovations: a new output block with room for the records, the old one freed only when everything is there
    filters_out_layout(f, B, f->innov, true);
    uint8_t *d_out = nullptr, *pin_out = nullptr;
    PhotoRec* d_part = nullptr;
    hipError_t e = hipMalloc((void**)&d_out, f->out_bytes);
    if (e == hipSuccess) e = hipHostMalloc((void**)&pin_out, f->out_bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void**)&d_part, photo_partial_count(B, 2 + f->iters) * sizeof(PhotoRec));
    if (e != hipSuccess) {
        if (d_out) (void)hipFree(d_out);
        if (pin_out) (void)hipHostFree(pin_out);
        if (d_part) (void)hipFree(d_part);
        filters_out_layout(f, B, f->innov, false);
        return fail(c, HNET_ERR_DEVICE, std::string("hnet_filters_enable_photometric: ") + hipGetErrorString(e));
    }
    (void)hipFree(f->d_out);
    (void)hipHostFree(f->pin_out);
    f->d_out = d_out;
    f->pin_out = pin_out;
    f->d_photo_part = d_part;
    f->last_n = 0;                                                 // what last_priors / last_selection / last_innovations described went with the old block
    f->last_innov_n = 0;
    f->last_photo_n = 0;
    std::fill(f->last_slot.begin(), f->last_slot.end(), -1);
    f->photo = true;
    return HNET_OK;
}

int hnet_filters_last_photometric(const hnet_filters* f, int n, hnet_photo_residual* out) {
    if (!f || !out) return HNET_ERR_INVALID_ARG;
    if (!f->photo || f->last_photo_n < 1) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_last_photometric: the last step ran without photometric records");
    if (n != f->last_photo_n) return fail(f->s->ctx, HNET_ERR_INVALID_ARG, "hnet_filters_last_photometric: n differs from the last step's");
    memcpy(out, f->pin_out + f->off_photo, (size_t)n * (2 + f->iters) * sizeof(PhotoRec));
    return HNET_OK;
}

// ---- filters, between frames (include/hnet.h): hnet_filters_predict.  Read-only: nothing of the filters' or the sessions' bookkeeping is written.

static_assert(sizeof(hnet_odometry) == sizeof(PredictOut), "hnet_odometry is the PredictOut layout");
static_assert(HNET_PRED_OK == PRED_OK && HNET_PRED_NO_STATE == PRED_NO_STATE && HNET_PRED_WAIT_IMU == PRED_WAIT_IMU && HNET_PRED_AT_STATE == PRED_AT_STATE,
              "HNET_PRED_* are the kernel's codes");

// the call's buffers, made once: the kernel's scratch is its own, so that hnet_filters_last_selection keeps describing the last advance
static int predict_buffers(hnet_filters* f) {
    if (f->d_pred) return HNET_OK;
    hnet_ctx* c = f->s->ctx;
    const int B = c->cfg.max_batch;
    f->off_pred_out = al256((size_t)B * sizeof(PredictJob));
    const size_t bytes = f->off_pred_out + (size_t)B * sizeof(PredictOut);
    hipError_t e = hipMalloc((void**)&f->d_pred_sel, (size_t)B * 2 * (f->cap + 2) * sizeof(hnet_ekf::ImuData));
    if (e == hipSuccess) e = hipHostMalloc((void**)&f->pin_pred, bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreate(&f->ev_p0);
    if (e == hipSuccess) e = hipEventCreate(&f->ev_p1);
    if (e == hipSuccess) e = hipMalloc((void**)&f->d_pred, bytes);
    if (e != hipSuccess) {
        if (f->d_pred_sel) (void)hipFree(f->d_pred_sel);
        if (f->pin_pred) (void)hipHostFree(f->pin_pred);
        if (f->ev_p0) (void)hipEventDestroy(f->ev_p0);
        if (f->ev_p1) (void)hipEventDestroy(f->ev_p1);
        f->d_pred_sel = nullptr; f->pin_pred = nullptr; f->ev_p0 = f->ev_p1 = nullptr; f->d_pred = nullptr;
        return fail(c, HNET_ERR_DEVICE, std::string("hnet_filters_predict: ") + hipGetErrorString(e));
    }
    return HNET_OK;
}

int hnet_filters_predict(hnet_filters* f, int n, const int32_t* ids, const double* t_query, hnet_odometry* out) {
    if (!f) return HNET_ERR_INVALID_ARG;
    hnet_sessions* s = f->s;
    hnet_ctx* c = s->ctx;
    if (!f->cap) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_predict: feed not enabled (hnet_filters_enable_feed)");
    if (!t_query || !out) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_predict: t_query / out");
    int rc = sessions_check_ids(s, n, ids);
    if (rc != HNET_OK) return rc;
    for (int i = 0; i < n; i++)
        if (!std::isfinite(t_query[i])) return fail(c, HNET_ERR_INVALID_ARG, "hnet_filters_predict: t_query must be finite");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    if ((rc = predict_buffers(f)) != HNET_OK) return rc;
    PredictJob* job = reinterpret_cast<PredictJob*>(f->pin_pred);
    for (int i = 0; i < n; i++) {
        const int id = ids[i];
        const double dt = f->cam_imu_dt[id];
        int st = PRED_OK;                                          // (the kernel reports AT_STATE from the device's own state time)
        if (!f->inited[id]) st = PRED_NO_STATE;
        else if (t_query[i] > f->t[id] && !(t_query[i] < f->imu_newest[id] - dt)) st = PRED_WAIT_IMU;
        job[i] = PredictJob{t_query[i], dt, id, st};
    }
    hipStream_t st = c->stream;
    PredictOut* d_out = reinterpret_cast<PredictOut*>(f->d_pred + f->off_pred_out);
    HIPCHK(c, hipMemcpyAsync(f->d_pred, f->pin_pred, (size_t)n * sizeof(PredictJob), hipMemcpyHostToDevice, st));
    if (f->pred_timed) HIPCHK(c, hipEventRecord(f->ev_p0, st));
    HIPCHK(c, launch_filter_predict(reinterpret_cast<const PredictJob*>(f->d_pred), n, s->n, f->cap, f->d_ring, f->d_meta, f->d_state, f->d_params, f->d_pred_sel,
                                    d_out, st));
    if (f->pred_timed) HIPCHK(c, hipEventRecord(f->ev_p1, st));
    HIPCHK(c, hipMemcpyAsync(f->pin_pred + f->off_pred_out, d_out, (size_t)n * sizeof(PredictOut), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    memcpy(out, f->pin_pred + f->off_pred_out, (size_t)n * sizeof(PredictOut));
    if (f->pred_timed) {
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, f->ev_p0, f->ev_p1));
        f->pred_ms = ms;
    }
    return HNET_OK;
}

double hnet_filters_newest_imu_time(const hnet_filters* f, int id) {
    if (!f || !f->cap || id < 0 || id >= f->s->n || !std::isfinite(f->imu_newest[id])) return NAN;
    return f->imu_newest[id];
}

double hnet_filters_last_predict_device_ms(hnet_filters* f) {
    if (!f) return NAN;
    f->pred_timed = true;
    return f->pred_ms;
}

}  // extern "C"
