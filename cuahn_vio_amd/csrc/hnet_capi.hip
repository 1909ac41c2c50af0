// hnet_capi.hip — the C ABI of include/hnet.h: contexts and groups, images and cameras, the inference entry points and the one policy that
// repairs their host results, timing and profiles, operator and debug entry points.
//
// Mirrors the behaviour of the reference runtime class pytorch::HomographyNet
// (cuahn_ros/homography_network/src/HomographyNet.cpp) without libtorch: weights come from an HNETW001
// blob, the forward is a fixed sequence of HIP kernel launches on one stream over persistent buffers.
#include "capi_internal.h"
#include "photo_masked_dev.h"

using namespace hnet;
using namespace capi;

// N contexts of one configuration on one device for INDEPENDENT steps (a server's batches, a rank's share of a streamed sequence): step k runs on context k mod N,
// each context on its own HIP stream, so that the dependent launch chain of one step runs under the kernels of the others.
struct hnet_group {
    std::vector<hnet_ctx*> ctx;
    std::vector<hipStream_t> streams;
    std::vector<hipEvent_t> ev;        // hnet_group_join: one event per member stream
    int device_id = 0;
    uint64_t next = 0;                 // round-robin position
    std::string err;
};

namespace {

const char* kStatus[] = {"ok", "invalid argument", "bad weights", "device error", "not ready (need two images)",
                         "batch exceeds max_batch", "unsupported"};

// Captures `body` (work enqueued on c->stream) into an executable graph.  Returns nullptr when capture is not possible;
// callers then fall back to eager launches of the same kernels.
template <class F>
hipGraphExec_t capture_graph(hnet_ctx* c, F&& body) {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) return nullptr;
    const int rc = body();
    const hipError_t e = hipStreamEndCapture(c->stream, &graph);
    if (rc != HNET_OK || e != hipSuccess || !graph) { if (graph) (void)hipGraphDestroy(graph); (void)hipGetLastError(); return nullptr; }
    if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) exec = nullptr;
    (void)hipGraphDestroy(graph);
    return exec;
}

// the whole weights file (the reference only prints on a load failure, HomographyNet.cpp:91-93; here it is an error code)
int read_weights_file(const char* path, const char* caller, std::vector<uint8_t>& buf) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "%s: cannot open weights file %s\n", caller, path); return HNET_ERR_BAD_WEIGHTS; }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    buf.assign(n > 0 ? n : 0, 0);
    const size_t got = n > 0 ? fread(buf.data(), 1, n, f) : 0;
    fclose(f);
    return (long)got == n ? HNET_OK : HNET_ERR_BAD_WEIGHTS;
}

int create_impl(const hnet_config* cfg_in, const uint8_t* blob, size_t len, hnet_ctx** out, hipStream_t preset_stream = nullptr) {
    if (!cfg_in || !out) return HNET_ERR_INVALID_ARG;
    hnet_config g;
    hnet_default_config(&g);
    memcpy(&g, cfg_in, std::min<size_t>(cfg_in->struct_size ? cfg_in->struct_size : sizeof(g), sizeof(g)));
    g.struct_size = sizeof(g);
    if (g.max_batch < 1) return HNET_ERR_INVALID_ARG;
    if (g.graph < HNET_GRAPH_DEFAULT || g.graph > HNET_GRAPH_TIMING) return HNET_ERR_INVALID_ARG;      // (unknown values no longer select the defaults silently)
    if (g.variant & ~(uint32_t)(HNET_VARIANT_GEMM_MASK | HNET_VARIANT_NO_LATENCY_PATH | HNET_VARIANT_UNFUSED_B3 | HNET_VARIANT_UNFUSED_B42 | HNET_VARIANT_NO_CHAIN | HNET_VARIANT_CHAIN_GRID_8 | HNET_VARIANT_CHAIN_GRID_3 | HNET_VARIANT_WARP_FUSE | HNET_VARIANT_GRAPH_COPIES | HNET_VARIANT_CHAIN_NO_FC)) return HNET_ERR_INVALID_ARG;
    {
        const uint32_t code = g.variant & HNET_VARIANT_GEMM_MASK;
        static const uint32_t known[] = {0, 13, 20, 21, 22, 25, 30};
        if (std::find(std::begin(known), std::end(known), code) == std::end(known)) return HNET_ERR_INVALID_ARG;
    }
    // the LDS-DMA / buffer-load kernels address an activation with 31-bit byte offsets (a buffer descriptor covers 2 GiB; an offset beyond it reads zeros,
    // silently).  The largest array is block_4_1's bordered map, B42_IMG x 16 channels x 2 bytes = 603 520 bytes per pair and plane, and block42_fused_kernel
    // reaches BOTH fp16 planes through one descriptor (lane offset = plane + patch chunk, scalar offset = tile origin): the sum of the two stays inside the
    // descriptor - whichever of them the hardware range-checks - for 2 x max_batch x 603 520 < 2^31 -> 1 779 pairs (round 4 bounded one plane: 3 558).
    // Larger batches: several calls.
    if ((size_t)2 * g.max_batch * B42_IMG * 32 >= ((size_t)1 << 31)) return HNET_ERR_CAPACITY;
    if (g.precision != HNET_PREC_FP32 && g.precision != HNET_PREC_BF16X3 && g.precision != HNET_PREC_BF16 && g.precision != HNET_PREC_F16X2)
        return HNET_ERR_UNSUPPORTED;
    Blob b;
    if (!parse_blob(blob, len, b)) return HNET_ERR_BAD_WEIGHTS;
    // the model variant: what the reference bakes into the traced .pt it loads (trace_model.py:16,36-46; HomographyNet.cpp:81-124 only names the file) comes from
    // the blob's `hnet.variant` record wherever the caller left the field at HNET_FROM_FILE; without a record, the reference's launch values
    {
        const Tensor* v = b.find("hnet.variant", {8});
        const bool rec = v && v->data[0] == 1.0f;
        if (v && !rec) return HNET_ERR_BAD_WEIGHTS;                       // a record version this library does not know
        // the record's numbers come from a file: finite, integral and in range BEFORE any float -> int conversion (a NaN or 1e30 there is undefined behaviour)
        int r_prior = 1, r_blocks = 3, r_mc = 16, r_err = 0;
        float r_p = 0.05f;
        if (rec) {
            auto rec_int = [&](int i, int lo, int hi, int& out) {
                const float f = v->data[i];
                if (!(f >= (float)lo && f <= (float)hi) || f != std::floor(f)) return false;
                out = (int)f;
                return true;
            };
            r_p = v->data[4];
            if (!rec_int(1, 0, 1, r_prior) || !rec_int(2, 1, 3, r_blocks) || !rec_int(3, 1, 256, r_mc) || !rec_int(5, 0, 1, r_err) || !(r_p >= 0.f && r_p < 1.f))
                return HNET_ERR_BAD_WEIGHTS;
        }
        if (g.use_prior == HNET_FROM_FILE) g.use_prior = r_prior;
        if (g.blocks_to_run == HNET_FROM_FILE) g.blocks_to_run = r_blocks;
        if (g.mc_samples == HNET_FROM_FILE) g.mc_samples = r_mc;
        if (g.dropout_p < 0.f) g.dropout_p = r_p;
        if (g.emit_error_map == HNET_FROM_FILE) g.emit_error_map = r_err;
    }
    if (g.mc_samples < 1 || g.mc_samples > 256 || !(g.dropout_p >= 0.f) || g.dropout_p >= 1.f || (g.use_prior != 0 && g.use_prior != 1) ||
        (g.emit_error_map != 0 && g.emit_error_map != 1))
        return HNET_ERR_INVALID_ARG;
    if (g.use_prior && (g.blocks_to_run < 1 || g.blocks_to_run > 3)) return HNET_ERR_INVALID_ARG;
    if ((size_t)g.max_batch * std::max((size_t)g.mc_samples * 1280, (size_t)4 * 5120) + 1024 >= ((size_t)1 << 32)) return HNET_ERR_CAPACITY;   // 32-bit indices of the keep-bit kernel (s3_dispatch.h)
    if (g.mc_sample_begin == 0 && g.mc_sample_end == 0) g.mc_sample_end = g.mc_samples;
    if (g.mc_sample_begin < 0 || g.mc_sample_end > g.mc_samples || g.mc_sample_begin >= g.mc_sample_end)
        return HNET_ERR_INVALID_ARG;

    if (g.precision == HNET_PREC_F16X2) {     // fp16 planes carry 4096 w: every matrix-core weight must stay below 16 (s3_format.h)
        float wmax = 0.f;
        for (int l = 0; l < 20; l++) {
            const ConvDesc& d = kConvs[l];
            const Tensor* w = b.find(std::string(d.block == 4 ? "model_last_block_list.0." : "model_part1.") + d.name + ".0.weight",
                                     {(uint32_t)d.cout, (uint32_t)d.cin, (uint32_t)d.ks, (uint32_t)d.ks});
            if (!w) return HNET_ERR_BAD_WEIGHTS;
            for (size_t i = 0; i < (size_t)d.cout * d.cin * d.ks * d.ks; i++) wmax = std::max(wmax, std::fabs(w->data[i]));
        }
        for (const char* head : {"fc_block_4_mean", "fc_block_4_uncertainty"}) {
            const Tensor* w = b.find(std::string("model_last_block_list.0.") + head + ".1.weight", {256, 5120});
            if (!w) return HNET_ERR_BAD_WEIGHTS;
            for (size_t i = 0; i < (size_t)256 * 5120; i++) wmax = std::max(wmax, std::fabs(w->data[i]));
        }
        if (!(wmax < 15.99f)) {    // same results, twice the matrix-core work: not an error
            fprintf(stderr, "hnet_create: HNET_PREC_F16X2 needs |weight| < 16 (largest here: %g): using HNET_PREC_BF16X3\n", wmax);
            g.precision = HNET_PREC_BF16X3;
        }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || g.device_id < 0 || g.device_id >= ndev) return HNET_ERR_DEVICE;
    hnet_ctx* c = new hnet_ctx();
    c->cfg = g;
    c->s3 = g.precision != HNET_PREC_FP32;   // the 16-bit matrix-core kernels; their arithmetic mode = the number of activation planes (s3_format.h)
    c->n_planes = g.precision == HNET_PREC_BF16 ? 1 : g.precision == HNET_PREC_F16X2 ? 2 : 3;
    // Kernel selection.  The library reads NO environment variable: what used to be HNET_* switches read at hnet_create (rounds 1 - 3) is either
    // gone with the kernels that lost ("Removed in round 4") or a documented field of hnet_config (warp_exact, graph, variant) that
    // the tests and tools/ab_bench.py set explicitly.
    c->fuse_b4 = c->s3;
    c->use_patch = c->s3;
    c->use_patch32 = true;
    c->warp_exact = g.warp_exact != 0;
    c->fuse_small = !(g.variant & HNET_VARIANT_NO_LATENCY_PATH);
    c->fuse_b3 = c->n_planes == 2 && !(g.variant & HNET_VARIANT_UNFUSED_B3);
    c->fuse_b42 = c->n_planes == 2 && !(g.variant & HNET_VARIANT_UNFUSED_B42);
    c->s3_tile = (int)(g.variant & HNET_VARIANT_GEMM_MASK);
    c->lat_tail = c->s3_tile != 30;                // (30: the splitk_reduce* launches and the split-K heads of rounds 1 - 4, A/B and bitwise tests)
    c->a14_pad = c->fuse_b4 && c->fuse_b42;
    c->patch_rb5 = 5;
    c->patch_b128 = true;
    c->b4_flags = 0;
    c->n_local = g.mc_sample_end - g.mc_sample_begin;
    c->s_begin = g.mc_sample_begin;
#define CK(expr)                                                                    \
    do {                                                                            \
        hipError_t e_ = (expr);                                                     \
        if (e_ != hipSuccess) {                                                     \
            fprintf(stderr, "hnet_create: %s: %s\n", #expr, hipGetErrorString(e_)); \
            hnet_destroy(c);                                                        \
            return HNET_ERR_DEVICE;                                                 \
        }                                                                           \
    } while (0)
    CK(hipSetDevice(g.device_id));
    CK(conv_kernels_init_device());      // dynamic-LDS limits of the patch / fused kernels: per device, so set at every create
    CK(chain_init_device());
    CK(photo_init_device());
    CK(photo_align_init_device());
    CK(photo_masked_init_device());
    if (preset_stream) { c->stream = preset_stream; c->owns_stream = false; }      // a group member: the group created its streams first, each on a priority level / hardware queue of its own
    else CK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    CK(hipEventCreate(&c->ev0));
    CK(hipEventCreate(&c->ev1));
    CK(hipEventCreate(&c->ev_align[0]));
    CK(hipEventCreate(&c->ev_align[1]));
    { const int rc_w = upload_weights(c, b); if (rc_w != HNET_OK) { hnet_destroy(c); return rc_w; } }
    if (c->n_planes == 2) c->blob_copy.assign(blob, blob + len);

    // ---- persistent activation buffers (NHWC fp32), one per layer so every intermediate can be read back
    const size_t MB = (size_t)g.max_batch;
    static const int first[4] = {0, 3, 7, 13}, last[4] = {2, 6, 12, 19};
    for (int blk = 0; blk < 4; blk++) {
        int h = IMG_H >> (3 - blk), w = IMG_W >> (3 - blk);
        CK(dalloc(&c->x_in[blk], MB * h * w * 2));
        for (int l = first[blk]; l <= last[blk]; l++) {
            h = conv_out_dim(h, kConvs[l].ks, kConvs[l].stride);
            w = conv_out_dim(w, kConvs[l].ks, kConvs[l].stride);
            c->act_c[l] = kConvs[l].cout; c->act_h[l] = h; c->act_w[l] = w;
            c->act_count[l] = (size_t)h * w * kConvs[l].cout;
            if (c->fuse_b4 && l == 13) continue;                   // block_4_0's output lives in LDS only (conv_b4_fused.h): 880 MB at batch 256 saved
            if (c->s3 && l == 14 && c->a14_pad) {                  // two bordered fp16 planes, or (after a demotion to split-bf16) three plain ones; the border stays zero
                const size_t bytes = std::max((size_t)3 * MB * c->act_count[l], (size_t)2 * MB * B42_IMG * 16) * 2;
                CK(hipMalloc((void**)&c->act16[l], bytes));
                CK(hipMemset(c->act16[l], 0, bytes));
            } else
            if (c->s3 && l != last[blk]) CK(hipMalloc((void**)&c->act16[l], 3 * MB * c->act_count[l] * 2));   // feeds a conv: S3 planes
            else CK(dalloc(&c->act[l], MB * c->act_count[l]));
        }
    }
    // measured on MI355X: graph replay 0.302 ms vs eager 0.292 ms per batch-1 forward - the batch-1 latency is device side
    // (45 short dependent kernels), not host launch cost, so replay is opt-in (HNET_GRAPH=1)
    // streaming entry point: one graph launch instead of ~43 kernel launches per frame: end-to-end p50 0.380 -> 0.334 ms
    // (device time of the forward 0.289 -> 0.300 ms)
    c->use_graph = g.graph != HNET_GRAPH_OFF;
    c->graph_timing = g.graph == HNET_GRAPH_TIMING;
    c->graph_zero_copy = !(g.variant & HNET_VARIANT_GRAPH_COPIES);
    CK(hipMalloc((void**)&c->d_seq, 8));
    CK(hipMemset(c->d_seq, 0, 8));
    CK(hipMalloc((void**)&c->d_flag, 4));
    CK(hipMemset(c->d_flag, 0, 4));
    CK(hipHostMalloc((void**)&c->pinned, sizeof(hnet_ctx::Pinned), hipHostMallocDefault));
    for (int i = 0; i < 2; i++) {
        CK(hipHostMalloc((void**)&c->pinned_img[i], NPIX, hipHostMallocDefault));
        CK(hipEventCreateWithFlags(&c->ev_img[i], hipEventDisableTiming));
    }
    if (c->fuse_b4) {                                        // zeroed once: the border is block_4_0's zero padding and is never written again
        c->x16_plane = MB * B4_HP * B4_WP;
        CK(hipMalloc((void**)&c->x16_b4, 3 * c->x16_plane * 4));
        CK(hipMemset(c->x16_b4, 0, 3 * c->x16_plane * 4));
    }
    // the one-XCD tail chains of the latency path (chain_lat.h): default mode only; variant 30 (the round-4 latency path) and NO_CHAIN keep the launches
    c->use_chain = c->n_planes == 2 && c->fuse_small && c->lat_tail && !(g.variant & HNET_VARIANT_NO_CHAIN);
    c->chain_grid = (g.variant & HNET_VARIANT_CHAIN_GRID_3) ? 3 : (g.variant & HNET_VARIANT_CHAIN_GRID_8) ? 8 : 256;
    // opt-in (it measured slower): block 4's warp + concat inside the block_4_0 + block_4_1 kernel (batch > 8): fp16-plane mode with the fast sampler
    c->warp_in = c->n_planes == 2 && c->fuse_b4 && c->x16_b4 && !c->warp_exact && (g.variant & HNET_VARIANT_WARP_FUSE);
    if (c->use_chain) {
        CK(hipMalloc((void**)&c->chain_sync, CH_AREAS * CH_SYNC_WORDS * sizeof(uint32_t)));
        CK(hipMemset(c->chain_sync, 0, CH_AREAS * CH_SYNC_WORDS * sizeof(uint32_t)));
        static const int chain_first[4] = {1, 4, 10, 17};
        ChainArgs* ca = c->chain_args;
        const bool chain_fc = !(g.variant & HNET_VARIANT_CHAIN_NO_FC);
        if (chain_fc) CK(dalloc(&c->fc_part, (size_t)CH_MAX_PAIRS * CH_FC_ITEMS * 8));
        for (int blk = 0; blk < 4; blk++) {
            for (int l = chain_first[blk], j = 0; l <= last[blk]; l++, j++) {
                ChainLayer& L = ca[blk].L[j];
                L.in = c->act16[l - 1]; L.in_plane = MB * c->act_count[l - 1];
                L.wfrag = c->chain_w[l]; L.bias = c->conv_b[l];
                L.out16 = c->act16[l]; L.out_plane = MB * c->act_count[l];
                L.out32 = c->act[l];
                if (!L.in || !L.wfrag || !(L.out16 || L.out32)) c->use_chain = false;      // (a layout this build does not expect: the launches)
            }
            ca[blk].flag = c->d_flag;
            ca[blk].fcw = nullptr; ca[blk].fc_part = nullptr;
            if (chain_fc && blk < 3 && c->fc_w[blk]) { ca[blk].fcw = c->fc_w[blk]; ca[blk].fc_part = c->fc_part; }      // the block-tail FC as partial sums of the last layer (chain_lat.h)
        }
    }
    c->ws_floats = (size_t)16 << 20;
    CK(dalloc(&c->ws, c->ws_floats + SPLITK_TICKETS));      // + the tile counters of the split-K launches (kernels.h): zero between launches
    CK(hipMemset(c->ws + c->ws_floats, 0, SPLITK_TICKETS * sizeof(uint32_t)));
    CK(dalloc(&c->hidden, MB * c->n_local * 512));
    if (c->s3) {
        CK(hipMalloc((void**)&c->feat16, 3 * MB * 5120 * 2));
        CK(hipMalloc((void**)&c->head_mask, MB * c->n_local * 2 * 640));
    }
    CK(dalloc(&c->Hm, MB * 9));
    CK(dalloc(&c->Hm2, MB * 9));
    CK(dalloc(&c->Htot, MB * 9));
    CK(dalloc(&c->mean_s, MB * c->n_local * 8));
    CK(dalloc(&c->logvar_s, MB * c->n_local * 8));
    CK(dalloc(&c->d_mean, MB * 8));
    CK(dalloc(&c->d_cov, MB * 64));
    CK(dalloc(&c->d_prior, MB * 8));
    CK(hipMalloc(&c->stage_prev, MB * NPIX * sizeof(float)));
    CK(hipMalloc(&c->stage_curr, MB * NPIX * sizeof(float)));
    if (g.emit_error_map) {
        CK(dalloc(&c->d_err, MB * NPIX));
        CK(dalloc(&c->d_err_u8, MB * NPIX));
    }
    CK(dalloc(&c->ring[0], (size_t)NPIX));
    CK(dalloc(&c->ring[1], (size_t)NPIX));
    build_stages(c, g.max_batch);

    // ---- warm-up forward on the reference's constant inputs (HomographyNet.cpp:28-45): 0.2 / 0.5 / prior 1.0
    {
        std::vector<float> i1(NPIX, 0.2f), i2(NPIX, 0.5f), pr(8, 1.0f);
        CK(hipMemcpy(c->stage_prev, i1.data(), NPIX * sizeof(float), hipMemcpyHostToDevice));
        CK(hipMemcpy(c->stage_curr, i2.data(), NPIX * sizeof(float), hipMemcpyHostToDevice));
        CK(hipMemcpy(c->d_prior, pr.data(), 8 * sizeof(float), hipMemcpyHostToDevice));
        const FwdArgs a{.prev = c->stage_prev, .curr = c->stage_curr, .pix_fmt = HNET_PIX_F32, .prior = g.use_prior ? c->d_prior : nullptr, .batch = 1,
                        .mean = c->d_mean, .cov = c->d_cov, .err = c->d_err};
        auto t0 = std::chrono::steady_clock::now();
        int rc = forward(c, a, c->stream);
        if (rc == HNET_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = HNET_ERR_DEVICE;
        if (rc != HNET_OK) {
            fprintf(stderr, "hnet_create: warm-up forward failed: %s\n", c->err.c_str());
            hnet_destroy(c);
            return rc;
        }
        c->timing.host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
#undef CK
    *out = c;
    return HNET_OK;
}

}  // namespace

namespace capi {

// `main_model`: the call the reference times (num_of_inference == 0, HomographyNet.cpp:174-189); IEKF re-runs (iteration > 0)
// advance the mask sequence number (n_inferences) but not the timing statistics (:245-251 sit under `num_of_inference == 0`)
void record_timing(hnet_timing& t, float dev_ms, double host_ms, int n_inferences, bool main_model) {
    t.device_ms = dev_ms;
    t.host_ms = host_ms;
    t.n_inferences += n_inferences;
    if (main_model) {
        t.n_main_inferences++;                                                  // inference_counting, :189
        if (t.n_main_inferences > 100) t.sum_device_ms_after_100 += dev_ms;     // :245-251
    }
}

// the captured forwards of hnet_infer and hnet_time_batch_device (they hold the kernels and buffers of the mode they were captured in)
static void drop_graphs(hnet_ctx* c) {
    for (auto& g : c->g_infer) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
    if (c->g_batch) { (void)hipGraphExecDestroy(c->g_batch); c->g_batch = nullptr; }
}

// HNET_PREC_F16X2 carries activations in fp16 planes (|a| < 32768 guaranteed, s3_format.h).  An overflow turns into infinities / NaNs that reach the outputs; the
// host-result entry points then re-pack the weights for HNET_PREC_BF16X3 (fp32 range, same kernels in their six-product form), run the call
// again and stay in that mode: a finite answer of the reference is never lost to the faster arithmetic.
static int demote_to_bf16x3(hnet_ctx* c) {
    if (c->n_planes != 2 || c->blob_copy.empty()) return HNET_ERR_UNSUPPORTED;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->ws) HIPCHK(c, hipMemset(c->ws + c->ws_floats, 0, SPLITK_TICKETS * sizeof(uint32_t)));      // the overflowed forward may have ended anywhere: counters back to zero
    Blob b;
    if (!parse_blob(c->blob_copy.data(), c->blob_copy.size(), b)) return fail(c, HNET_ERR_BAD_WEIGHTS, "weight blob");
    c->n_planes = 3;
    c->use_chain = false;
    c->warp_in = false;
    c->fuse_b3 = c->fuse_b42 = c->a14_pad = false;    // the fused block-3 / block_4_2+4_3 kernels exist for the fp16 planes only (their layers' buffers stay allocated; act16[14] goes back to the plain layout)
    c->cfg.precision = HNET_PREC_BF16X3;
    const int rc = upload_weights(c, b);
    if (rc != HNET_OK) return fail(c, rc, "re-packing the weights for HNET_PREC_BF16X3");
    drop_graphs(c);
    c->blob_copy.clear();
    c->blob_copy.shrink_to_fit();
    build_stages(c, c->cfg.max_batch);     // the fused fp16-plane kernels are gone from the launch list
    fprintf(stderr, "hnet: activation beyond the fp16 range in HNET_PREC_F16X2: context demoted to HNET_PREC_BF16X3\n");
    return HNET_OK;
}
// A bounded spin of a one-XCD tail chain gave up (chain_lat.h CH_FLAG_TIMEOUT in the flag word: a claimed item never completed - not observed; the bound exists so
// that a scheduling surprise ends in a flagged forward instead of a hung device).  The context goes back to the launches for good; the host entry points repeat the call.
static int chain_gave_up(hnet_ctx* c) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->use_chain = false;
    if (c->chain_sync) HIPCHK(c, hipMemset(c->chain_sync, 0, CH_AREAS * CH_SYNC_WORDS * sizeof(uint32_t)));
    drop_graphs(c);
    build_stages(c, c->cfg.max_batch);
    fprintf(stderr, "hnet: a tail-chain launch timed out on its in-launch hand-off: this context uses the per-layer launches from now on\n");
    return HNET_OK;
}

// The policy of every entry point that returns its results to the host (hnet_infer, hnet_infer_batch, hnet_sessions_infer[_iter], hnet_filters_step,
// hnet_filters_advance).  ctx[0] is the call's context (its stream carries the work), ctx[1] a second context whose forwards the same attempt enqueues
// on that stream (the sessions' iterative model), or null.  `enqueue` runs one complete attempt: its work, the download of the results and of the flag
// word of every context that ran (flag[k] of ctx[k]; 0 for one that did not), the reset of those words, the synchronisation.  A tail chain that timed
// out sends the context that flagged it back to the launches and the attempt runs again; then, on the latest results, an fp16-plane overflow
// (`overflowed`: the index of the context whose forward gave non-finite outputs of finite inputs, -1 for none; the entry point's own test) demotes
// that context and the attempt runs again - a context demotes once, so two contexts repeat twice at the most.  The caller advances its counters once,
// after an accepted call.  A failed attempt may leave copies from pinned buffers in flight: the stream is drained before the error returns.
int run_host_call(hnet_ctx* const ctx[2], const std::function<int(uint32_t* flag)>& enqueue, const std::function<int()>& overflowed) {
    uint32_t flag[2] = {0, 0};
    int rc = enqueue(flag);
    bool again = false;
    for (int k = 0; k < 2 && rc == HNET_OK; k++)
        if (ctx[k] && (flag[k] & CH_FLAG_TIMEOUT) && (rc = chain_gave_up(ctx[k])) == HNET_OK) again = true;
    if (rc == HNET_OK && again) rc = enqueue(flag);
    auto f16 = [&](int k) { return k >= 0 && ctx[k] && ctx[k]->n_planes == 2; };
    for (int k; rc == HNET_OK && (f16(0) || f16(1)) && f16(k = overflowed());)
        if ((rc = demote_to_bf16x3(ctx[k])) == HNET_OK) rc = enqueue(flag);
    if (rc != HNET_OK) (void)hipStreamSynchronize(ctx[0]->stream);
    return rc;
}

// initialize_undist_map[_fisheye] (CamBase.h:165-180): the maps of `cam` (hnet_set_camera, hnet_sessions_add_camera)
void build_undistort_maps(const hnet_camera* cam, std::vector<float>& mx, std::vector<float>& my) {
    // the virtual camera every frame is resampled to: 90 deg horizontal field of view on 320 px (CamBase.h:166-169)
    const double f = (IMG_W - 1.0) / 2.0 / std::tan(45.0 / 180.0 * (2.0 * std::acos(0.0)));
    const double cx = (IMG_W - 1.0) / 2.0, cy = (IMG_H - 1.0) / 2.0;
    mx.assign(NPIX, 0.0f);
    my.assign(NPIX, 0.0f);
    for (int v = 0; v < IMG_H; v++)
        for (int u = 0; u < IMG_W; u++) {
            const double x = (u - cx) / f, y = (v - cy) / f;          // R = I: the pixel's ray in the virtual camera
            double xd, yd;
            if (cam->fisheye) {                                      // cv::fisheye::initUndistortRectifyMap (equidistant)
                const double r = std::sqrt(x * x + y * y), th = std::atan(r), t2 = th * th;
                const double thd = th * (1.0 + t2 * (cam->d[0] + t2 * (cam->d[1] + t2 * (cam->d[2] + t2 * cam->d[3]))));
                const double sc = r == 0.0 ? 1.0 : thd / r;
                xd = x * sc; yd = y * sc;
            } else {                                                 // cv::initUndistortRectifyMap, D = (k1, k2, p1, p2)
                const double r2 = x * x + y * y, kr = 1.0 + r2 * (cam->d[0] + r2 * cam->d[1]);
                xd = x * kr + 2.0 * cam->d[2] * x * y + cam->d[3] * (r2 + 2.0 * x * x);
                yd = y * kr + cam->d[2] * (r2 + 2.0 * y * y) + 2.0 * cam->d[3] * x * y;
            }
            mx[v * IMG_W + u] = (float)(cam->k[0] * xd + cam->k[2]);
            my[v * IMG_W + u] = (float)(cam->k[1] * yd + cam->k[3]);
        }
}

}  // namespace capi

extern "C" {

void hnet_default_config(hnet_config* cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = sizeof(*cfg);
    cfg->blocks_to_run = 3;
    cfg->mc_samples = 16;        // model_to_trace.py:202
    cfg->dropout_p = 0.05f;      // trace_model.py:16
    cfg->precision = HNET_PREC_F16X2;    // fp32-grade results on the fp16 matrix cores, three MFMAs per product (same parity tests as HNET_PREC_BF16X3 / FP32)
    cfg->max_batch = 1;
}

int hnet_create_from_memory(const hnet_config* cfg, const void* blob, size_t len, hnet_ctx** out) {
    if (!blob) return HNET_ERR_INVALID_ARG;
    return create_impl(cfg, (const uint8_t*)blob, len, out);
}

int hnet_create(const hnet_config* cfg, const char* weights_path, hnet_ctx** out) {
    if (!weights_path) return HNET_ERR_INVALID_ARG;
    std::vector<uint8_t> buf;
    const int rc = read_weights_file(weights_path, "hnet_create", buf);
    return rc != HNET_OK ? rc : create_impl(cfg, buf.data(), buf.size(), out);
}

// ---- context groups
static int create_group_impl(const hnet_config* cfg, const uint8_t* blob, size_t len, int n_ctx, hnet_group** out) {
    if (!cfg || !out || n_ctx < 1 || n_ctx > HNET_GROUP_MAX) return HNET_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device_id < 0 || cfg->device_id >= ndev) return HNET_ERR_DEVICE;
    if (hipSetDevice(cfg->device_id) != hipSuccess) return HNET_ERR_DEVICE;
    hnet_group* g = new hnet_group();
    g->device_id = cfg->device_id;
    // The streams FIRST, in a fixed order, before any other stream of the group exists, and each on its own priority level as far as the device has levels: the
    // HIP runtime multiplexes the streams of ONE priority over its hardware queues (which queue a stream gets depends on every stream the process created before),
    // and two member streams that share a queue serialise their steps; queues of different priority are never shared.
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);          // numerically: greatest <= least (lower = more urgent)
    const int levels = least - greatest + 1;
    for (int i = 0; i < n_ctx; i++) {
        hipStream_t st = nullptr;
        const int prio = levels > 1 ? greatest + (i % levels) : 0;
        if (hipStreamCreateWithPriority(&st, hipStreamNonBlocking, prio) != hipSuccess) { hnet_destroy_group(g); return HNET_ERR_DEVICE; }
        g->streams.push_back(st);
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { hnet_destroy_group(g); return HNET_ERR_DEVICE; }
        g->ev.push_back(e);
    }
    for (int i = 0; i < n_ctx; i++) {
        hnet_ctx* c = nullptr;
        const int rc = create_impl(cfg, blob, len, &c, g->streams[i]);
        if (rc != HNET_OK) { hnet_destroy_group(g); return rc; }
        g->ctx.push_back(c);
    }
    *out = g;
    return HNET_OK;
}

int hnet_create_group_from_memory(const hnet_config* cfg, const void* blob, size_t len, int n_ctx, hnet_group** out) {
    if (!blob) return HNET_ERR_INVALID_ARG;
    return create_group_impl(cfg, (const uint8_t*)blob, len, n_ctx, out);
}

int hnet_create_group(const hnet_config* cfg, const char* weights_path, int n_ctx, hnet_group** out) {
    if (!weights_path) return HNET_ERR_INVALID_ARG;
    std::vector<uint8_t> buf;
    const int rc = read_weights_file(weights_path, "hnet_create_group", buf);
    return rc != HNET_OK ? rc : create_group_impl(cfg, buf.data(), buf.size(), n_ctx, out);
}

void hnet_destroy_group(hnet_group* g) {
    if (!g) return;
    (void)hipSetDevice(g->device_id);
    for (hnet_ctx* c : g->ctx) hnet_destroy(c);                          // (synchronises the member's stream; the streams are the group's)
    for (hipEvent_t e : g->ev) if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : g->streams) if (s) (void)hipStreamDestroy(s);
    delete g;
}

int hnet_group_size(const hnet_group* g) { return g ? (int)g->ctx.size() : 0; }
hnet_ctx* hnet_group_context(hnet_group* g, int i) { return (g && i >= 0 && i < (int)g->ctx.size()) ? g->ctx[i] : nullptr; }
void* hnet_group_stream(hnet_group* g, int i) { return (g && i >= 0 && i < (int)g->streams.size()) ? (void*)g->streams[i] : nullptr; }
const char* hnet_group_last_error(const hnet_group* g) { return g ? g->err.c_str() : ""; }

int hnet_group_infer_batch_packed_device(hnet_group* g, const void* d_prev, const void* d_curr, int pix_fmt, const float* d_prior, int batch, uint64_t pair_seq0,
                                         float* d_out72, float* d_err_map, int* member) {
    if (!g || g->ctx.empty()) return HNET_ERR_INVALID_ARG;
    const int i = (int)(g->next % g->ctx.size());
    const int rc = hnet_infer_batch_packed_device(g->ctx[i], d_prev, d_curr, pix_fmt, d_prior, batch, pair_seq0, d_out72, d_err_map, nullptr);
    if (rc != HNET_OK) { g->err = g->ctx[i]->err; return rc; }
    g->next++;
    if (member) *member = i;
    return HNET_OK;
}

int hnet_group_join(hnet_group* g, void* stream) {
    if (!g || !stream) return HNET_ERR_INVALID_ARG;
    if (hipSetDevice(g->device_id) != hipSuccess) return HNET_ERR_DEVICE;
    for (size_t i = 0; i < g->streams.size(); i++) {
        if (hipEventRecord(g->ev[i], g->streams[i]) != hipSuccess || hipStreamWaitEvent((hipStream_t)stream, g->ev[i], 0) != hipSuccess) {
            g->err = "hnet_group_join: event";
            return HNET_ERR_DEVICE;
        }
    }
    return HNET_OK;
}

int hnet_group_synchronize(hnet_group* g) {
    if (!g) return HNET_ERR_INVALID_ARG;
    if (hipSetDevice(g->device_id) != hipSuccess) return HNET_ERR_DEVICE;
    for (hipStream_t s : g->streams)
        if (hipStreamSynchronize(s) != hipSuccess) { g->err = "hipStreamSynchronize"; return HNET_ERR_DEVICE; }
    return HNET_OK;
}

int hnet_group_overflow_flag(hnet_group* g, int* flags) {
    if (!g || !flags) return HNET_ERR_INVALID_ARG;
    int all = 0;
    for (hnet_ctx* c : g->ctx) {
        int f = 0;
        const int rc = hnet_overflow_flag(c, nullptr, &f);
        if (rc != HNET_OK) { g->err = c->err; return rc; }
        all |= f;
    }
    *flags = all;
    return HNET_OK;
}

void hnet_destroy(hnet_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->cfg.device_id);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    auto fr = [](void* p) { if (p) (void)hipFree(p); };
    for (int l = 0; l < 20; l++) { fr(c->patch_frag[l]); fr(c->conv_w[l]); fr(c->conv_b[l]); fr(c->act[l]); fr(c->conv_w16[l]); fr(c->conv_wfrag[l]); fr(c->act16[l]); }
    for (int k = 0; k < 3; k++) { fr(c->fc_w[k]); fr(c->fc_b[k]); }
    for (int k = 0; k < 4; k++) fr(c->x_in[k]);
    drop_graphs(c);
    if (c->pinned) (void)hipHostFree(c->pinned);
    for (int i = 0; i < 2; i++) {
        if (c->pinned_img[i]) (void)hipHostFree(c->pinned_img[i]);
        if (c->ev_img[i]) (void)hipEventDestroy(c->ev_img[i]);
    }
    fr(c->d_seq); fr(c->d_flag); fr(c->chain_sync); fr(c->fc_part);
    for (int l = 0; l < 20; l++) fr(c->chain_w[l]);
    fr(c->und_map[0]); fr(c->und_map[1]); fr(c->raw_dev);
    fr(c->s2_frag[0]); fr(c->s2_frag[3]); fr(c->x16_b4); fr(c->b30_frag); fr(c->b40_frag); fr(c->b41_frag); fr(c->w1_16); fr(c->b3f_w1); fr(c->b42_w2); fr(c->b42_w3); fr(c->feat16); fr(c->head_mask);
    fr(c->ws); fr(c->w1); fr(c->b1); fr(c->w2); fr(c->b2); fr(c->hidden); fr(c->Hm); fr(c->Hm2); fr(c->Htot); fr(c->mean_s); fr(c->logvar_s);
    fr(c->d_mean); fr(c->d_cov); fr(c->d_err); fr(c->d_err_u8); fr(c->d_prior); fr(c->stage_prev); fr(c->stage_curr); fr(c->pyr_scratch);
    fr(c->ring[0]); fr(c->ring[1]);
    for (auto e : c->prof_ev) (void)hipEventDestroy(e);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (hipEvent_t e : c->ev_align) if (e) (void)hipEventDestroy(e);
    if (c->stream && c->owns_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* hnet_status_string(int s) { return (s >= 0 && s <= 6) ? kStatus[s] : "unknown status"; }
const char* hnet_last_error(const hnet_ctx* c) { return c ? c->err.c_str() : ""; }
const char* hnet_version(void) { return "hnet-hip 0.1.0 (gfx950)"; }

int hnet_push_image(hnet_ctx* c, const uint8_t* data, int rows, int cols, int row_stride, double t) {
    if (!c || !data) return HNET_ERR_INVALID_ARG;
    if (rows != IMG_H || cols != IMG_W || row_stride < cols) return fail(c, HNET_ERR_INVALID_ARG, "image must be 224x320 8-bit");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    c->img_counter++;                                               // HomographyNet.cpp:134
    const int slot = c->img_counter == 1 ? 0 : (c->curr_slot ^ 1);  // prev <- curr: flip the ring instead of cloning (:143)
    // `data` is not retained (the cv::Mat may be reused): copy it into a pinned staging frame and upload from there without
    // waiting; network_inference follows on the same stream.  The staging frame of this slot was last used two pushes ago.
    HIPCHK(c, hipEventSynchronize(c->ev_img[slot]));
    for (int r = 0; r < IMG_H; r++) memcpy(c->pinned_img[slot] + (size_t)r * IMG_W, data + (size_t)r * row_stride, IMG_W);
    HIPCHK(c, hipMemcpyAsync(c->ring[slot], c->pinned_img[slot], NPIX, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_img[slot], c->stream));
    c->curr_slot = slot;
    if (c->img_counter >= 2) c->latest_t = t;                       // :148
    return HNET_OK;
}

// ---- image pre-processing: CamBase.h:165-186
int hnet_set_undistort_maps(hnet_ctx* c, const float* map_x, const float* map_y, int raw_rows, int raw_cols) {
    if (!c || !map_x || !map_y || raw_rows < 1 || raw_cols < 1 || raw_rows > 16384 || raw_cols > 16384) return HNET_ERR_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    for (int i = 0; i < 2; i++)
        if (!c->und_map[i]) HIPCHK(c, dalloc(&c->und_map[i], (size_t)NPIX));
    HIPCHK(c, hipMemcpy(c->und_map[0], map_x, NPIX * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->und_map[1], map_y, NPIX * 4, hipMemcpyHostToDevice));
    if (c->raw_dev && (size_t)raw_rows * raw_cols > (size_t)c->raw_rows * c->raw_cols) { (void)hipFree(c->raw_dev); c->raw_dev = nullptr; }
    if (!c->raw_dev) HIPCHK(c, hipMalloc((void**)&c->raw_dev, (size_t)raw_rows * raw_cols));
    c->raw_rows = raw_rows;
    c->raw_cols = raw_cols;
    return HNET_OK;
}

int hnet_set_camera(hnet_ctx* c, const hnet_camera* cam) {
    if (!c || !cam) return HNET_ERR_INVALID_ARG;
    std::vector<float> mx, my;
    build_undistort_maps(cam, mx, my);
    return hnet_set_undistort_maps(c, mx.data(), my.data(), cam->raw_rows, cam->raw_cols);
}

int hnet_get_undistort_maps(hnet_ctx* c, float* map_x, float* map_y) {
    if (!c || !map_x || !map_y) return HNET_ERR_INVALID_ARG;
    if (!c->und_map[0]) return fail(c, HNET_ERR_NOT_READY, "no camera set");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipMemcpy(map_x, c->und_map[0], NPIX * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(map_y, c->und_map[1], NPIX * 4, hipMemcpyDeviceToHost));
    return HNET_OK;
}

static int remap_raw(hnet_ctx* c, const uint8_t* raw, int rows, int cols, int row_stride, uint8_t* d_out) {
    if (!c->und_map[0]) return fail(c, HNET_ERR_NOT_READY, "hnet_set_camera / hnet_set_undistort_maps first");
    if (rows != c->raw_rows || cols != c->raw_cols || row_stride < cols) return fail(c, HNET_ERR_INVALID_ARG, "raw image size differs from the camera's");
    HIPCHK(c, hipMemcpy2DAsync(c->raw_dev, cols, raw, row_stride, cols, rows, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_undistort(c->raw_dev, rows, cols, cols, c->und_map[0], c->und_map[1], d_out, c->stream));
    return HNET_OK;
}

int hnet_push_raw_image(hnet_ctx* c, const uint8_t* raw, int rows, int cols, int row_stride, double t) {
    if (!c || !raw) return HNET_ERR_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const int slot = c->img_counter == 0 ? 0 : (c->curr_slot ^ 1);
    const int rc = remap_raw(c, raw, rows, cols, row_stride, c->ring[slot]);
    if (rc != HNET_OK) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));                     // `raw` is not retained
    c->img_counter++;
    c->curr_slot = slot;
    if (c->img_counter >= 2) c->latest_t = t;
    return HNET_OK;
}

int hnet_op_undistort(hnet_ctx* c, const uint8_t* raw, int rows, int cols, int row_stride, uint8_t* out) {
    if (!c || !raw || !out) return HNET_ERR_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    DevTemps t;
    uint8_t* d_o = nullptr;
    HIPCHK(c, t.alloc(&d_o, (size_t)NPIX));
    const int rc = remap_raw(c, raw, rows, cols, row_stride, d_o);
    if (rc == HNET_OK) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(out, d_o, NPIX, hipMemcpyDeviceToHost));
    }
    return rc;
}

int hnet_image_count(const hnet_ctx* c) { return c ? (c->img_src ? c->img_src : c)->img_counter : 0; }
double hnet_latest_time(const hnet_ctx* c) { return c ? (c->img_src ? c->img_src : c)->latest_t : -1.0; }

int hnet_precision(const hnet_ctx* c) { return c ? c->cfg.precision : -1; }
int hnet_get_config(const hnet_ctx* c, hnet_config* out) {
    if (!c || !out) return HNET_ERR_INVALID_ARG;
    *out = c->cfg;
    return HNET_OK;
}

int hnet_overflow_flag(hnet_ctx* c, void* stream, int* flags) {
    if (!c || !flags) return HNET_ERR_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    uint32_t v = 0;
    HIPCHK(c, hipMemcpyAsync(&v, c->d_flag, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemsetAsync(c->d_flag, 0, 4, s));
    HIPCHK(c, hipStreamSynchronize(s));
    *flags = (int)v;
    return HNET_OK;
}

int hnet_infer(hnet_ctx* c, const double* prior_px, int iteration, float mean_out[8], float cov_out[64], uint8_t* err_map_out) {
    if (!c || !mean_out || !cov_out) return HNET_ERR_INVALID_ARG;
    hnet_ctx* src = c->img_src ? c->img_src : c;                 // the context that owns the frames and the sequence count (hnet_attach_images)
    if (src->img_counter < 2) return fail(c, HNET_ERR_NOT_READY, "HNet cannot inference! Only has one image!");   // :155-158
    if (err_map_out && !c->cfg.emit_error_map) return fail(c, HNET_ERR_INVALID_ARG, "context was created without emit_error_map");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    auto t0 = std::chrono::steady_clock::now();
    if (c->cfg.use_prior && !prior_px) return fail(c, HNET_ERR_INVALID_ARG, "prior required");
    if (src != c) HIPCHK(c, hipStreamWaitEvent(c->stream, src->ev_img[src->curr_slot], 0));      // the frame's upload runs on the source's stream
    hnet_ctx::Pinned* pin = c->pinned;
    auto enqueue = [&](uint32_t& flag_now) -> int {
        const int slot = src->curr_slot;
        if (c->use_graph && !c->g_infer[slot]) {
            // one graph per ring orientation (captured again after a repair dropped it).  Round 6: no memcpy nodes - the pinned host block is mapped into the
            // device's address space and the kernels read the sequence number and the prior from it and write mean, covariance, error map and the flag word to it
            // (six copy / memset nodes of 3 - 8 us each in a chain of 16 launches; HNET_VARIANT_GRAPH_COPIES keeps them: H2D {seq, prior} -> forward -> D2H {mean, cov, err, flag})
            hnet_ctx::Pinned* dpin = nullptr;
            if (c->graph_zero_copy && hipHostGetDevicePointer((void**)&dpin, pin, 0) != hipSuccess) { (void)hipGetLastError(); c->graph_zero_copy = false; }
            c->g_infer[slot] = capture_graph(c, [&]() -> int {
                if (c->graph_zero_copy)
                    return forward(c, FwdArgs{.prev = src->ring[slot ^ 1], .curr = src->ring[slot], .prior = c->cfg.use_prior ? dpin->prior : nullptr, .batch = 1, .mean = dpin->mean,
                                              .cov = dpin->cov, .err_u8 = c->cfg.emit_error_map ? dpin->err : nullptr, .seq_dev = &dpin->seq, .flag = &dpin->flag}, c->stream);
                if (hipMemcpyAsync(c->d_seq, &pin->seq, 8, hipMemcpyHostToDevice, c->stream) != hipSuccess) return HNET_ERR_DEVICE;
                if (c->cfg.use_prior && hipMemcpyAsync(c->d_prior, pin->prior, 32, hipMemcpyHostToDevice, c->stream) != hipSuccess) return HNET_ERR_DEVICE;
                const int rc = forward(c, FwdArgs{.prev = src->ring[slot ^ 1], .curr = src->ring[slot], .prior = c->cfg.use_prior ? c->d_prior : nullptr, .batch = 1,
                                                  .mean = c->d_mean, .cov = c->d_cov, .err_u8 = c->cfg.emit_error_map ? c->d_err_u8 : nullptr, .seq_dev = c->d_seq}, c->stream);
                if (rc != HNET_OK) return rc;
                if (hipMemcpyAsync(pin->mean, c->d_mean, 32, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return HNET_ERR_DEVICE;
                if (hipMemcpyAsync(pin->cov, c->d_cov, 256, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return HNET_ERR_DEVICE;
                if (c->cfg.emit_error_map && hipMemcpyAsync(pin->err, c->d_err_u8, NPIX, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return HNET_ERR_DEVICE;
                if (hipMemcpyAsync(&pin->flag, c->d_flag, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return HNET_ERR_DEVICE;
                // the host entry points inspect (and, for an overflow, repair) their own results: the device flag is for the device-resident entry points only
                if (hipMemsetAsync(c->d_flag, 0, 4, c->stream) != hipSuccess) return HNET_ERR_DEVICE;
                return HNET_OK;
            });
            if (!c->g_infer[slot]) c->use_graph = false;      // capture unavailable: eager launches below, same kernels
            c->g_infer_H[slot] = c->H_last;
        }
        if (c->use_graph && c->g_infer[slot]) {
            c->H_last = c->g_infer_H[slot];
            pin->seq = (uint64_t)src->timing.n_inferences;
            if (c->cfg.use_prior) for (int i = 0; i < 8; i++) pin->prior[i] = (float)prior_px[i];    // :160-165 toType(kFloat)
            if (c->graph_zero_copy) pin->flag = 0;                 // (raised by the kernels directly; the memcpy form overwrites it)
            HIPCHK(c, hipEventRecord(c->ev0, c->stream));
            HIPCHK(c, hipGraphLaunch(c->g_infer[slot], c->stream));
            HIPCHK(c, hipEventRecord(c->ev1, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            memcpy(mean_out, pin->mean, 32);
            memcpy(cov_out, pin->cov, 256);
            if (err_map_out) memcpy(err_map_out, pin->err, NPIX);
            flag_now = pin->flag;
            return HNET_OK;
        }
        if (c->cfg.use_prior) {
            float pf[8];
            for (int i = 0; i < 8; i++) pf[i] = (float)prior_px[i];    // :160-165 toType(kFloat)
            HIPCHK(c, hipMemcpyAsync(c->d_prior, pf, sizeof pf, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        const FwdArgs a{.prev = src->ring[slot ^ 1], .curr = src->ring[slot], .prior = c->cfg.use_prior ? c->d_prior : nullptr, .batch = 1,
                        .seq0 = (uint64_t)src->timing.n_inferences, .mean = c->d_mean, .cov = c->d_cov, .err_u8 = err_map_out ? c->d_err_u8 : nullptr};
        HIPCHK(c, hipEventRecord(c->ev0, c->stream));
        const int rc = forward(c, a, c->stream);
        if (rc != HNET_OK) return rc;
        HIPCHK(c, hipEventRecord(c->ev1, c->stream));
        HIPCHK(c, hipMemcpyAsync(mean_out, c->d_mean, 8 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(cov_out, c->d_cov, 64 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        if (err_map_out) HIPCHK(c, hipMemcpyAsync(err_map_out, c->d_err_u8, NPIX, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&flag_now, c->d_flag, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_flag, 0, 4, c->stream));      // (see the graph's capture)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return HNET_OK;
    };
    const int rc = run_host_call(c, enqueue, [&] {
        return !(all_finite(mean_out, 8) && all_finite(cov_out, 64)) && all_finite(c->cfg.use_prior ? prior_px : nullptr, 8);
    });
    if (rc != HNET_OK) return rc;
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    record_timing(c->timing, ms, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), 1, iteration == 0);
    if (src != c) src->timing.n_inferences++;             // one shared sequence count
    return HNET_OK;
}

int hnet_attach_images(hnet_ctx* c, hnet_ctx* source) {
    if (!c || !source || c == source || source->img_src) return HNET_ERR_INVALID_ARG;
    if (c->cfg.device_id != source->cfg.device_id) return fail(c, HNET_ERR_INVALID_ARG, "hnet_attach_images: both contexts must live on one device");
    c->img_src = source;
    return HNET_OK;
}

// the checks the device-resident forward entry points share (`args_ok`: their own pointer arguments; `check_fmt` false: hnet_infer_mc_partial_device,
// which passes the pixel format on unchecked), and the stream they enqueue on
static int device_entry(hnet_ctx* c, bool args_ok, int pix_fmt, const float* d_err_map, void* stream, hipStream_t& s, bool check_fmt = true) {
    if (!c || !args_ok) return HNET_ERR_INVALID_ARG;
    if (check_fmt && pix_fmt != HNET_PIX_U8 && pix_fmt != HNET_PIX_F32) return fail(c, HNET_ERR_INVALID_ARG, "pix_fmt");
    if (d_err_map && !c->cfg.emit_error_map) return fail(c, HNET_ERR_INVALID_ARG, "context was created without emit_error_map");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    s = stream ? (hipStream_t)stream : c->stream;
    return HNET_OK;
}

int hnet_infer_batch_device(hnet_ctx* c, const void* d_prev, const void* d_curr, int pix_fmt, const float* d_prior, int batch,
                            uint64_t pair_seq0, float* d_mean, float* d_cov, float* d_err_map, void* stream) {
    hipStream_t s = nullptr;
    const int rc = device_entry(c, d_prev && d_curr && d_mean && d_cov, pix_fmt, d_err_map, stream, s);
    return rc != HNET_OK ? rc : forward(c, FwdArgs{.prev = d_prev, .curr = d_curr, .pix_fmt = pix_fmt, .prior = d_prior, .batch = batch, .seq0 = pair_seq0,
                                                   .mean = d_mean, .cov = d_cov, .err = d_err_map}, s);
}

int hnet_infer_batch_packed_device(hnet_ctx* c, const void* d_prev, const void* d_curr, int pix_fmt, const float* d_prior, int batch,
                                   uint64_t pair_seq0, float* d_out72, float* d_err_map, void* stream) {
    hipStream_t s = nullptr;
    const int rc = device_entry(c, d_prev && d_curr && d_out72, pix_fmt, d_err_map, stream, s);
    return rc != HNET_OK ? rc : forward(c, FwdArgs{.prev = d_prev, .curr = d_curr, .pix_fmt = pix_fmt, .prior = d_prior, .batch = batch, .seq0 = pair_seq0,
                                                   .mean = d_out72, .cov = d_out72 + 8, .err = d_err_map,
                                                   .mean_stride = HNET_PACKED_FLOATS, .cov_stride = HNET_PACKED_FLOATS}, s);
}

int hnet_infer_batch(hnet_ctx* c, const void* prev, const void* curr, int pix_fmt, const float* prior, int batch,
                     uint64_t pair_seq0, float* mean, float* cov, float* err_map) {
    if (!c || !prev || !curr || !mean || !cov) return HNET_ERR_INVALID_ARG;
    if (pix_fmt != HNET_PIX_U8 && pix_fmt != HNET_PIX_F32) return fail(c, HNET_ERR_INVALID_ARG, "pix_fmt");
    if (batch < 1) return fail(c, HNET_ERR_INVALID_ARG, "batch < 1");
    if (batch > c->cfg.max_batch) return fail(c, HNET_ERR_CAPACITY, "batch exceeds max_batch");
    if (err_map && !c->cfg.emit_error_map) return fail(c, HNET_ERR_INVALID_ARG, "context was created without emit_error_map");
    if (c->cfg.use_prior && !prior) return fail(c, HNET_ERR_INVALID_ARG, "prior required");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    auto t0 = std::chrono::steady_clock::now();
    const size_t px = pix_fmt == HNET_PIX_U8 ? 1 : 4;
    hipStream_t s = c->stream;
    const FwdArgs a{.prev = c->stage_prev, .curr = c->stage_curr, .pix_fmt = pix_fmt, .prior = prior ? c->d_prior : nullptr, .batch = batch, .seq0 = pair_seq0,
                    .mean = c->d_mean, .cov = c->d_cov, .err = err_map ? c->d_err : nullptr};
    auto enqueue = [&](uint32_t& flag_now) -> int {
        HIPCHK(c, hipMemcpyAsync(c->stage_prev, prev, (size_t)batch * NPIX * px, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(c->stage_curr, curr, (size_t)batch * NPIX * px, hipMemcpyHostToDevice, s));
        if (prior) HIPCHK(c, hipMemcpyAsync(c->d_prior, prior, (size_t)batch * 8 * sizeof(float), hipMemcpyHostToDevice, s));
        HIPCHK(c, hipEventRecord(c->ev0, s));
        const int rc = forward(c, a, s);
        if (rc != HNET_OK) return rc;
        HIPCHK(c, hipEventRecord(c->ev1, s));
        HIPCHK(c, hipMemcpyAsync(mean, c->d_mean, (size_t)batch * 8 * sizeof(float), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(cov, c->d_cov, (size_t)batch * 64 * sizeof(float), hipMemcpyDeviceToHost, s));
        if (err_map) HIPCHK(c, hipMemcpyAsync(err_map, c->d_err, (size_t)batch * NPIX * sizeof(float), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(&flag_now, c->d_flag, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemsetAsync(c->d_flag, 0, 4, s));              // host results are inspected by run_host_call: hnet_overflow_flag reports device-resident batches only
        HIPCHK(c, hipStreamSynchronize(s));
        return HNET_OK;
    };
    const int rc = run_host_call(c, enqueue, [&] {
        return !(all_finite(mean, (size_t)batch * 8) && all_finite(cov, (size_t)batch * 64)) && (!prior || all_finite(prior, (size_t)batch * 8)) &&
               (pix_fmt == HNET_PIX_U8 || (all_finite((const float*)prev, (size_t)batch * NPIX) && all_finite((const float*)curr, (size_t)batch * NPIX)));
    });
    if (rc != HNET_OK) return rc;
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    record_timing(c->timing, ms, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), 1, true);
    return HNET_OK;
}

int hnet_infer_mc_partial_device(hnet_ctx* c, const void* d_prev, const void* d_curr, int pix_fmt, const float* d_prior,
                                 int batch, uint64_t pair_seq0, float* d_mean_s, float* d_logvar_s, float* d_h_part1, void* stream) {
    hipStream_t s = nullptr;
    const int rc = device_entry(c, d_prev && d_curr && d_mean_s && d_logvar_s, pix_fmt, nullptr, stream, s, false);
    return rc != HNET_OK ? rc : forward(c, FwdArgs{.prev = d_prev, .curr = d_curr, .pix_fmt = pix_fmt, .prior = d_prior, .batch = batch, .seq0 = pair_seq0,
                                                   .mean_s = d_mean_s, .logvar_s = d_logvar_s, .h_part1 = d_h_part1, .partial = true}, s);
}

int hnet_mc_finish_device(hnet_ctx* c, const float* d_mean_s, const float* d_logvar_s, int n_total, const float* d_h_part1,
                          int batch, float* d_mean, float* d_cov, void* stream) {
    if (!c || !d_mean_s || !d_logvar_s || !d_h_part1 || !d_mean || !d_cov || n_total < 1 || batch < 1) return HNET_ERR_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, launch_mc_finish(d_mean_s, d_logvar_s, n_total, d_h_part1, batch, d_mean, d_cov, nullptr,
                               stream ? (hipStream_t)stream : c->stream, c->d_flag));
    return HNET_OK;
}

int hnet_mc_finish_packed_device(hnet_ctx* c, const float* d_mean_s, const float* d_logvar_s, int n_total, const float* d_h_part1,
                                 int batch, float* d_out72, void* stream) {
    if (!c || !d_mean_s || !d_logvar_s || !d_h_part1 || !d_out72 || n_total < 1 || batch < 1) return HNET_ERR_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, launch_mc_finish(d_mean_s, d_logvar_s, n_total, d_h_part1, batch, d_out72, d_out72 + 8, nullptr,
                               stream ? (hipStream_t)stream : c->stream, c->d_flag, HNET_PACKED_FLOATS, HNET_PACKED_FLOATS));
    return HNET_OK;
}

int hnet_mc_finish_gathered_device(hnet_ctx* c, const float* d_gathered, int world, int n_local, const float* d_h_part1, int batch, float* d_out72, void* stream) {
    if (!c || !d_gathered || !d_h_part1 || !d_out72 || world < 1 || n_local < 1 || batch < 1) return HNET_ERR_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const size_t block = (size_t)batch * n_local * 8;        // floats of one [B][n_local][8] array; a rank's message is [mean block | log-variance block]
    HIPCHK(c, launch_mc_finish(d_gathered, d_gathered + block, world * n_local, d_h_part1, batch, d_out72, d_out72 + 8, nullptr,
                               stream ? (hipStream_t)stream : c->stream, c->d_flag, HNET_PACKED_FLOATS, HNET_PACKED_FLOATS, n_local, 2 * block));
    return HNET_OK;
}

int hnet_synchronize(hnet_ctx* c, void* stream) {
    if (!c) return HNET_ERR_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipStreamSynchronize(stream ? (hipStream_t)stream : c->stream));
    return HNET_OK;
}

int hnet_last_timing(const hnet_ctx* c, hnet_timing* out) {
    if (!c || !out) return HNET_ERR_INVALID_ARG;
    *out = c->timing;
    return HNET_OK;
}

int hnet_time_batch_device(hnet_ctx* c, const void* d_prev, const void* d_curr, int pix_fmt, const float* d_prior, int batch,
                           uint64_t pair_seq0, float* d_mean, float* d_cov, int iters, float* per_iter_ms, float* total_ms) {
    if (!c || iters < 1) return HNET_ERR_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    std::vector<hipEvent_t> ev(iters + 1);
    for (auto& e : ev) HIPCHK(c, hipEventCreate(&e));
    int rc = HNET_OK;
    // small batches: replay the forward as one hipGraph (what hnet_infer does); the mask sequence number is refreshed
    // from pinned memory once before the timed loop (every replay then uses the same masks - timing only)
    hipGraphExec_t gx = nullptr;
    if (c->graph_timing && c->use_graph && batch <= 8) {
        hnet_ctx::GraphKey key = {d_prev, d_curr, d_prior, d_mean, d_cov, batch, pix_fmt};
        if (!(c->g_batch && key == c->g_key)) {
            if (c->g_batch) { (void)hipGraphExecDestroy(c->g_batch); c->g_batch = nullptr; }
            c->g_batch = capture_graph(c, [&]() -> int {
                if (hipMemcpyAsync(c->d_seq, &c->pinned->seq, 8, hipMemcpyHostToDevice, c->stream) != hipSuccess) return HNET_ERR_DEVICE;
                return forward(c, FwdArgs{.prev = d_prev, .curr = d_curr, .pix_fmt = pix_fmt, .prior = d_prior, .batch = batch, .mean = d_mean, .cov = d_cov,
                                          .seq_dev = c->d_seq}, c->stream);
            });
            c->g_key = key;
            c->g_batch_H = c->H_last;
        }
        gx = c->g_batch;
        if (gx) { c->pinned->seq = pair_seq0; c->H_last = c->g_batch_H; }
    }
    HIPCHK(c, hipEventRecord(ev[0], c->stream));
    for (int i = 0; i < iters && rc == HNET_OK; i++) {
        if (gx) { if (hipGraphLaunch(gx, c->stream) != hipSuccess) rc = fail(c, HNET_ERR_DEVICE, "hipGraphLaunch"); }
        else rc = hnet_infer_batch_device(c, d_prev, d_curr, pix_fmt, d_prior, batch, pair_seq0 + (uint64_t)i * batch, d_mean, d_cov, nullptr, nullptr);
        if (rc == HNET_OK && hipEventRecord(ev[i + 1], c->stream) != hipSuccess) rc = fail(c, HNET_ERR_DEVICE, "hipEventRecord");
    }
    if (rc == HNET_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, HNET_ERR_DEVICE, "hipStreamSynchronize");
    if (rc == HNET_OK) {
        for (int i = 0; i < iters; i++) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
            if (per_iter_ms) per_iter_ms[i] = ms;
        }
        if (total_ms) (void)hipEventElapsedTime(total_ms, ev[0], ev[iters]);
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    return rc;
}

/* ---- per-stage (per kernel launch) device timing with HIP events on the context stream ---- */
int hnet_stage_count(const hnet_ctx* c) { return c ? (int)c->stages.size() : 0; }
const char* hnet_stage_name(const hnet_ctx* c, int i) { return (c && i >= 0 && i < (int)c->stages.size()) ? c->stages[i].name.c_str() : ""; }
int hnet_stage_kernels(const hnet_ctx* c, int i) { return (c && i >= 0 && i < (int)c->stages.size()) ? c->stages[i].kernels : 0; }
double hnet_stage_flops_per_pair(const hnet_ctx* c, int i) { return (c && i >= 0 && i < (int)c->stages.size()) ? c->stages[i].flops_per_pair : 0.0; }

int hnet_profile_batch_device(hnet_ctx* c, const void* d_prev, const void* d_curr, int pix_fmt, const float* d_prior, int batch,
                              uint64_t pair_seq0, float* d_mean, float* d_cov, int iters, float* stage_ms_avg) {
    if (!c || iters < 1 || !stage_ms_avg) return HNET_ERR_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    build_stages(c, batch, d_prev, d_curr, pix_fmt);   // the launches of a forward of THIS batch and THESE images (the latency path has fewer): hnet_stage_name follows
    const size_t ns = c->stages.size();
    std::vector<double> acc(ns, 0.0);
    // the per-stage events live in the context only for the duration of this call: whatever happens, they are destroyed
    // and the list is emptied again (a non-empty list makes every later forward single-stream and event-recording)
    struct Cleanup {
        hnet_ctx* c;
        ~Cleanup() { for (auto e : c->prof_ev) if (e) (void)hipEventDestroy(e); c->prof_ev.clear(); c->prof_pos = 0; }
    } cleanup{c};
    c->prof_ev.assign(ns, nullptr);
    for (auto& e : c->prof_ev) HIPCHK(c, hipEventCreate(&e));
    for (int it = 0; it < iters; it++) {
        c->prof_pos = 0;
        HIPCHK(c, hipEventRecord(c->ev0, c->stream));
        const int rc = hnet_infer_batch_device(c, d_prev, d_curr, pix_fmt, d_prior, batch, pair_seq0, d_mean, d_cov,
                                               c->cfg.emit_error_map ? c->d_err : nullptr, nullptr);
        if (rc != HNET_OK) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        hipEvent_t prev = c->ev0;
        for (size_t i = 0; i < c->prof_pos; i++) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, prev, c->prof_ev[i]);
            acc[i] += ms;
            prev = c->prof_ev[i];
        }
    }
    for (size_t i = 0; i < ns; i++) stage_ms_avg[i] = (float)(acc[i] / iters);
    return HNET_OK;
}

/* ---- operator-level entry points (host buffers) ---- */
int hnet_op_warp(hnet_ctx* c, const float* img, const float* H, float* out) {
    if (!c || !img || !H || !out) return HNET_ERR_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    DevTemps t;
    float *d_i = nullptr, *d_o = nullptr, *d_h = nullptr;
    HIPCHK(c, t.alloc(&d_i, (size_t)NPIX)); HIPCHK(c, t.alloc(&d_o, (size_t)NPIX)); HIPCHK(c, t.alloc(&d_h, (size_t)9));
    HIPCHK(c, hipMemcpy(d_i, img, NPIX * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_h, H, 36, hipMemcpyHostToDevice));
    HIPCHK(c, launch_warp_f32(d_i, d_h, d_o, 1, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, d_o, NPIX * 4, hipMemcpyDeviceToHost));
    return HNET_OK;
}

int hnet_op_dlt(hnet_ctx* c, const float* dst, int n, float* H) {
    if (!c || !dst || !H || n < 1) return HNET_ERR_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    DevTemps t;
    float *d_d = nullptr, *d_h = nullptr;
    HIPCHK(c, t.alloc(&d_d, (size_t)n * 8)); HIPCHK(c, t.alloc(&d_h, (size_t)n * 9));
    HIPCHK(c, hipMemcpy(d_d, dst, (size_t)n * 32, hipMemcpyHostToDevice));
    HIPCHK(c, launch_dlt(d_d, d_h, n, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(H, d_h, (size_t)n * 36, hipMemcpyDeviceToHost));
    return HNET_OK;
}

static_assert(sizeof(hnet_photo_residual) == sizeof(PhotoRec) && (int)HNET_PHOTO_DEGENERATE == PHOTO_DEGENERATE && (int)HNET_PHOTO_MAX_CANDIDATES == PHOTO_MAX_CAND,
              "hnet_photo_residual is the PhotoRec layout");

// photometric residual records of n host frame pairs under m candidate offset vectors each (csrc/kernels_photo.hip): ONE upload {img1 | img2 | offsets},
// the kernel and its slice sum, ONE download {records | map}, one synchronisation
int hnet_op_photo_residual(hnet_ctx* c, const uint8_t* img1, const uint8_t* img2, int n, const float* offsets_px, int m, hnet_photo_residual* out, float* map_out) {
    if (!c) return HNET_ERR_INVALID_ARG;
    if (!img1 || !img2 || !offsets_px || !out || n < 1 || m < 1 || m > PHOTO_MAX_CAND) return fail(c, HNET_ERR_INVALID_ARG, "hnet_op_photo_residual: frames / offsets / out, n >= 1, 1 <= m <= 66");
    if (n > c->cfg.max_batch) return fail(c, HNET_ERR_CAPACITY, "hnet_op_photo_residual: n exceeds max_batch");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const size_t img = (size_t)n * NPIX, off_bytes = (size_t)n * m * 8 * sizeof(float), up = 2 * img + off_bytes;            // (NPIX is a multiple of 16: every section stays aligned)
    const size_t rec_bytes = ((size_t)n * m * sizeof(PhotoRec) + 15) & ~(size_t)15, map_bytes = map_out ? (size_t)n * m * NPIX * sizeof(float) : 0;
    DevTemps t;
    uint8_t *d_in = nullptr, *d_res = nullptr;
    PhotoRec* d_part = nullptr;
    HIPCHK(c, t.alloc(&d_in, up));
    HIPCHK(c, t.alloc(&d_res, rec_bytes + map_bytes));
    HIPCHK(c, t.alloc(&d_part, photo_partial_count(n, m)));
    std::vector<uint8_t> h_in(up), h_res(rec_bytes + map_bytes);
    memcpy(h_in.data(), img1, img);
    memcpy(h_in.data() + img, img2, img);
    memcpy(h_in.data() + 2 * img, offsets_px, off_bytes);
    HIPCHK(c, hipMemcpyAsync(d_in, h_in.data(), up, hipMemcpyHostToDevice, c->stream));
    const PhotoCands cands{reinterpret_cast<const float*>(d_in + 2 * img), nullptr, nullptr, 0};
    HIPCHK(c, launch_photo_residual(d_in, d_in + img, n, cands, m, d_part, reinterpret_cast<PhotoRec*>(d_res), map_out ? reinterpret_cast<float*>(d_res + rec_bytes) : nullptr, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_res.data(), d_res, rec_bytes + map_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(out, h_res.data(), (size_t)n * m * sizeof(PhotoRec));
    if (map_out) memcpy(map_out, h_res.data() + rec_bytes, map_bytes);
    return HNET_OK;
}

// operator level: levels 1 .. 3 of n host frames -> out [n][PYR_BYTES]
int hnet_op_photo_pyramid(hnet_ctx* c, const uint8_t* img, int n, uint8_t* out) {
    if (!c) return HNET_ERR_INVALID_ARG;
    if (!img || !out || n < 1) return fail(c, HNET_ERR_INVALID_ARG, "hnet_op_photo_pyramid: frames / out, n >= 1");
    if (n > c->cfg.max_batch) return fail(c, HNET_ERR_CAPACITY, "hnet_op_photo_pyramid: n exceeds max_batch");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    DevTemps t;
    uint8_t *d_in = nullptr, *d_out = nullptr;
    HIPCHK(c, t.alloc(&d_in, (size_t)n * NPIX));
    HIPCHK(c, t.alloc(&d_out, (size_t)n * PYR_BYTES));
    std::vector<uint8_t> h_out((size_t)n * PYR_BYTES);
    HIPCHK(c, hipMemcpyAsync(d_in, img, (size_t)n * NPIX, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_photo_pyramid(d_in, nullptr, n, d_out, nullptr, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_out.data(), d_out, h_out.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(out, h_out.data(), h_out.size());
    return HNET_OK;
}

// the end of the layer-level operator entry points: n_out floats of the device result d_d to the host
static int op_result(hnet_ctx* c, float* out, const float* d_d, size_t n_out) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, d_d, n_out * 4, hipMemcpyDeviceToHost));
    return HNET_OK;
}

int hnet_op_conv(hnet_ctx* c, int layer, const float* in, int batch, int h, int w, float* out) {
    if (!c || !in || !out || layer < 0 || layer >= 20 || batch < 1 || h < 1 || w < 1) return HNET_ERR_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const ConvDesc& d = kConvs[layer];
    const int ho = conv_out_dim(h, d.ks, d.stride), wo = conv_out_dim(w, d.ks, d.stride);
    const size_t n_in = (size_t)batch * d.cin * h * w, n_out = (size_t)batch * d.cout * ho * wo;
    DevTemps t;
    float *d_a = nullptr, *d_b = nullptr, *d_c = nullptr, *d_d = nullptr;
    HIPCHK(c, t.alloc(&d_a, n_in)); HIPCHK(c, t.alloc(&d_b, n_in)); HIPCHK(c, t.alloc(&d_c, n_out)); HIPCHK(c, t.alloc(&d_d, n_out));
    HIPCHK(c, hipMemcpy(d_a, in, n_in * 4, hipMemcpyHostToDevice));
    if (!c->s3) {
        HIPCHK(c, launch_nchw_to_nhwc(d_a, d_b, batch, d.cin, h, w, c->stream));
        HIPCHK(c, launch_conv(layer, d_b, batch, h, w, c->conv_w[layer], c->conv_b[layer], d_c, c->stream));
        HIPCHK(c, launch_nhwc_to_nchw(d_c, d_d, batch, d.cout, ho, wo, c->stream));
    } else {   // split-bf16 mode: the layer reads / writes three bf16 planes, exactly as inside the forward
        uint16_t *p_in = nullptr, *p_out = nullptr;
        int out_np = c->n_planes;            // plane format p_out is written in
        HIPCHK(c, t.alloc(&p_in, 3 * n_in + 32));
        HIPCHK(c, t.alloc(&p_out, 3 * n_out + 32));
        if (c->use_patch && (conv_is_patch_layer(layer) || (c->use_patch32 && conv_is_patch32_layer(layer) && h == 56 && w == 80))) {
            HIPCHK(c, launch_nchw_f32_to_nhwc_s3(d_a, p_in, n_in, batch, d.cin, h, w, c->stream, c->n_planes));
            HIPCHK(c, launch_conv_patch(layer, p_in, n_in, batch, h, w, c->patch_frag[layer], c->conv_b[layer], p_out, n_out, c->stream, c->n_planes, c->patch_b128, c->patch_rb5));
        } else if (conv_is_s3_layer(layer)) {
            HIPCHK(c, launch_nchw_f32_to_nhwc_s3(d_a, p_in, n_in, batch, d.cin, h, w, c->stream, c->n_planes));
            HIPCHK(c, launch_conv_s3(layer, p_in, n_in, batch, h, w, c->conv_w16[layer], (size_t)d.cout * conv_padded_k(layer),
                                     c->conv_b[layer], p_out, n_out, nullptr, c->stream, nullptr, 0, c->conv_wfrag[layer], c->n_planes, c->s3_tile));
        } else {
            HIPCHK(c, launch_nchw_to_nhwc(d_a, d_b, batch, d.cin, h, w, c->stream));
            if (conv_is_first_s2(layer) && c->first_s2 && c->s2_frag[layer] && h == (layer == 0 ? 28 : 56) && w == (layer == 0 ? 40 : 80))
                HIPCHK(c, launch_conv_first_s2(layer, d_b, c->s2_frag[layer], c->conv_b[layer], p_out, n_out, batch, c->stream, c->n_planes));
            else if (layer == 7 && c->b30_s3 && c->b30_frag)     // the kernel the forward uses for block_3_0
                HIPCHK(c, launch_conv_first_s3(d_b, c->b30_frag, c->conv_b[layer], p_out, n_out, batch, h, w, c->stream, c->n_planes));
            else {   // Cin = 2 layers at other geometries: the fp32-MFMA kernel, which writes three bf16 planes
                HIPCHK(c, launch_conv(layer, d_b, batch, h, w, c->conv_w[layer], c->conv_b[layer], nullptr, c->stream, nullptr, 0, p_out, n_out));
                if (out_np == 2) out_np = 3;
            }
        }
        HIPCHK(c, launch_nhwc_s3_to_nchw_f32(p_out, n_out, d_d, batch, d.cout, ho, wo, c->stream, out_np));
    }
    return op_result(c, out, d_d, n_out);
}

int hnet_op_block4_fused(hnet_ctx* c, const float* in, int batch, int reverse, float* out) {
    if (!c || !in || !out || batch < 1) return HNET_ERR_INVALID_ARG;
    if (!c->fuse_b4 || !c->b40_frag || !c->b41_frag) return fail(c, HNET_ERR_UNSUPPORTED, "the fused block_4_0 + block_4_1 kernel exists in the split-bf16 mode only");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const size_t n_in = (size_t)batch * 2 * NPIX, n_out = (size_t)batch * 16 * (IMG_H / 2) * (IMG_W / 2);
    DevTemps t;
    float *d_a = nullptr, *d_b = nullptr, *d_d = nullptr;
    uint16_t* p_out = nullptr;
    HIPCHK(c, t.alloc(&d_a, n_in)); HIPCHK(c, t.alloc(&d_b, n_in)); HIPCHK(c, t.alloc(&d_d, n_out)); HIPCHK(c, t.alloc(&p_out, 3 * n_out + 32));
    HIPCHK(c, hipMemcpy(d_a, in, n_in * 4, hipMemcpyHostToDevice));
    HIPCHK(c, launch_nchw_to_nhwc(d_a, d_b, batch, 2, IMG_H, IMG_W, c->stream));
    const void* x_in = d_b;
    size_t x_plane = 0;
    {                                    // the kernel reads padded 16-bit planes with a zero border
        uint32_t* d_p = nullptr;
        x_plane = (size_t)batch * B4_HP * B4_WP;
        HIPCHK(c, t.alloc(&d_p, 3 * x_plane));
        HIPCHK(c, hipMemsetAsync(d_p, 0, 3 * x_plane * 4, c->stream));
        HIPCHK(c, launch_f32_nhwc_to_s3pad(d_b, d_p, x_plane, batch, c->n_planes, c->stream));
        x_in = d_p;
    }
    HIPCHK(c, launch_block4_fused(x_in, x_plane, c->b40_frag, c->conv_b[13], c->b41_frag, c->conv_b[14], p_out, n_out, batch, c->stream, (reverse ? 1 : 0) | (c->b4_flags & 32),
                                  c->n_planes));
    HIPCHK(c, launch_nhwc_s3_to_nchw_f32(p_out, n_out, d_d, batch, 16, IMG_H / 2, IMG_W / 2, c->stream, c->n_planes));
    return op_result(c, out, d_d, n_out);
}

int hnet_op_block42_fused(hnet_ctx* c, const float* in, int batch, float* out) {
    if (!c || !in || !out || batch < 1) return HNET_ERR_INVALID_ARG;
    if (!c->fuse_b42 || !c->b42_w2 || !c->b42_w3) return fail(c, HNET_ERR_UNSUPPORTED, "the fused block_4_2 + block_4_3 kernel exists in the fp16-plane mode only");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const int h1 = IMG_H / 2, w1 = IMG_W / 2;
    const size_t n_in = (size_t)batch * 16 * h1 * w1, n_out = (size_t)batch * 64 * (h1 / 4) * (w1 / 4);
    DevTemps t;
    float *d_a = nullptr, *d_d = nullptr;
    uint16_t *p_in = nullptr, *p_out = nullptr;
    HIPCHK(c, t.alloc(&d_a, n_in)); HIPCHK(c, t.alloc(&d_d, n_out)); HIPCHK(c, t.alloc(&p_in, 3 * n_in + 32)); HIPCHK(c, t.alloc(&p_out, 3 * n_out + 32));
    HIPCHK(c, hipMemcpy(d_a, in, n_in * 4, hipMemcpyHostToDevice));
    HIPCHK(c, launch_nchw_f32_to_nhwc_s3(d_a, p_in, n_in, batch, 16, h1, w1, c->stream, c->n_planes));
    uint16_t* p_pad = nullptr;                     // the kernel's input layout: planes with a zero border (kernels.h B42_*)
    const size_t n_pad = (size_t)batch * B42_IMG * 16;
    HIPCHK(c, t.alloc(&p_pad, 2 * n_pad));
    HIPCHK(c, hipMemsetAsync(p_pad, 0, 2 * n_pad * 2, c->stream));
    HIPCHK(c, launch_s3_repitch(p_in, n_in, p_pad, n_pad, batch, h1, w1, 16, B42_HP, B42_WP, B42_PADY, B42_PADX, true, c->stream, 2));
    HIPCHK(c, launch_block42_fused(p_pad, n_pad, c->b42_w2, c->conv_b[15], c->b42_w3, c->conv_b[16], p_out, n_out, batch, c->stream, c->n_planes));
    HIPCHK(c, launch_nhwc_s3_to_nchw_f32(p_out, n_out, d_d, batch, 64, h1 / 4, w1 / 4, c->stream, c->n_planes));
    return op_result(c, out, d_d, n_out);
}

int hnet_op_block3_fused(hnet_ctx* c, const float* in, int batch, float* out) {
    if (!c || !in || !out || batch < 1) return HNET_ERR_INVALID_ARG;
    if (!c->fuse_b3 || !c->b30_frag || !c->b3f_w1) return fail(c, HNET_ERR_UNSUPPORTED, "the fused block_3_0 + block_3_1 kernel exists in the fp16-plane mode only");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const int h0 = IMG_H / 2, w0 = IMG_W / 2;
    const size_t n_in = (size_t)batch * 2 * h0 * w0, n_out = (size_t)batch * 32 * (h0 / 2) * (w0 / 2);
    DevTemps t;
    float *d_a = nullptr, *d_b = nullptr, *d_d = nullptr;
    uint16_t* p_out = nullptr;
    HIPCHK(c, t.alloc(&d_a, n_in)); HIPCHK(c, t.alloc(&d_b, n_in)); HIPCHK(c, t.alloc(&d_d, n_out)); HIPCHK(c, t.alloc(&p_out, 3 * n_out + 32));
    HIPCHK(c, hipMemcpy(d_a, in, n_in * 4, hipMemcpyHostToDevice));
    HIPCHK(c, launch_nchw_to_nhwc(d_a, d_b, batch, 2, h0, w0, c->stream));
    HIPCHK(c, launch_block3_fused(d_b, c->b30_frag, c->conv_b[7], c->b3f_w1, c->conv_b[8], p_out, n_out, batch, c->stream, c->n_planes));
    HIPCHK(c, launch_nhwc_s3_to_nchw_f32(p_out, n_out, d_d, batch, 32, h0 / 2, w0 / 2, c->stream, c->n_planes));
    return op_result(c, out, d_d, n_out);
}

static int op_prep_impl(hnet_ctx* c, const void* img1, const void* img2, int pix_fmt, const float* H, int k, float* out) {
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const int ho = IMG_H / k, wo = IMG_W / k;
    const size_t px = pix_fmt == HNET_PIX_U8 ? 1 : 4;
    DevTemps t;
    uint8_t *d_1 = nullptr, *d_2 = nullptr;
    float *d_h = nullptr, *d_o = nullptr, *d_t = nullptr;
    HIPCHK(c, t.alloc(&d_1, NPIX * px)); HIPCHK(c, t.alloc(&d_2, NPIX * px)); HIPCHK(c, t.alloc(&d_h, (size_t)9));
    HIPCHK(c, t.alloc(&d_o, (size_t)2 * ho * wo)); HIPCHK(c, t.alloc(&d_t, (size_t)2 * ho * wo));
    HIPCHK(c, hipMemcpy(d_1, img1, NPIX * px, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_2, img2, NPIX * px, hipMemcpyHostToDevice));
    if (H) HIPCHK(c, hipMemcpy(d_h, H, 36, hipMemcpyHostToDevice));
    HIPCHK(c, launch_prep(d_1, d_2, pix_fmt, H ? d_h : nullptr, k, d_o, 1, c->stream, nullptr, 0, 3, c->warp_exact));
    HIPCHK(c, launch_nhwc_to_nchw(d_o, d_t, 1, 2, ho, wo, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, d_t, (size_t)2 * ho * wo * 4, hipMemcpyDeviceToHost));
    return HNET_OK;
}

int hnet_op_prep(hnet_ctx* c, const float* img1, const float* img2, const float* H, int k, float* out) {
    if (!c || !img1 || !img2 || !out || (k != 1 && k != 2 && k != 4 && k != 8)) return HNET_ERR_INVALID_ARG;
    return op_prep_impl(c, img1, img2, HNET_PIX_F32, H, k, out);
}

int hnet_op_prep_u8(hnet_ctx* c, const uint8_t* img1, const uint8_t* img2, const float* H, int k, float* out) {
    if (!c || !img1 || !img2 || !out || (k != 1 && k != 2 && k != 4 && k != 8)) return HNET_ERR_INVALID_ARG;
    return op_prep_impl(c, img1, img2, HNET_PIX_U8, H, k, out);
}

// A batch of pairs through ONE launch_prep, as the forward issues it (batch = n, the context's sampler, optionally the block-4 planes): the frames are
// uploaded align_off bytes past a 16-byte boundary, so that the tiled kernels (16-byte aligned frames) and the direct-gather routes can both be reached.
int hnet_op_prep_batch(hnet_ctx* c, const void* img1, const void* img2, int pix_fmt, const float* H, int n, int k, int align_off, float* out, uint32_t* planes) {
    if (!c) return HNET_ERR_INVALID_ARG;
    if (!img1 || !img2 || !out || n < 1 || n > 4096 || (k != 1 && k != 2 && k != 4 && k != 8) || (pix_fmt != HNET_PIX_U8 && pix_fmt != HNET_PIX_F32) ||
        align_off < 0 || align_off > 15)
        return fail(c, HNET_ERR_INVALID_ARG, "hnet_op_prep_batch: frames / out, 1 <= n <= 4096, k in {1, 2, 4, 8}, a pixel format, 0 <= align_off <= 15");
    if (pix_fmt == HNET_PIX_F32 && (align_off & 3)) return fail(c, HNET_ERR_INVALID_ARG, "hnet_op_prep_batch: float frames need an align_off that is a multiple of 4");
    if (planes && (k != 1 || !H)) return fail(c, HNET_ERR_INVALID_ARG, "hnet_op_prep_batch: the block-4 planes exist for k = 1 with a homography only");
    if (planes && !c->x16_b4) return fail(c, HNET_ERR_UNSUPPORTED, "hnet_op_prep_batch: this context's forward has no block-4 plane input");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const int ho = IMG_H / k, wo = IMG_W / k;
    const size_t px = pix_fmt == HNET_PIX_U8 ? 1 : 4, img_bytes = (size_t)n * NPIX * px, n_out = (size_t)n * 2 * ho * wo;
    const size_t plane = (size_t)n * B4_HP * B4_WP;                         // dwords per plane
    DevTemps t;
    uint8_t *d_1 = nullptr, *d_2 = nullptr;
    float *d_h = nullptr, *d_o = nullptr, *d_t = nullptr;
    uint32_t* d_p = nullptr;
    HIPCHK(c, t.alloc(&d_1, img_bytes + 16)); HIPCHK(c, t.alloc(&d_2, img_bytes + 16)); HIPCHK(c, t.alloc(&d_h, (size_t)n * 9));
    HIPCHK(c, t.alloc(&d_o, n_out)); HIPCHK(c, t.alloc(&d_t, n_out));
    if ((((uintptr_t)d_1 | (uintptr_t)d_2) & 15) != 0) return fail(c, HNET_ERR_DEVICE, "hnet_op_prep_batch: a device allocation is not 16-byte aligned");
    HIPCHK(c, hipMemcpy(d_1 + align_off, img1, img_bytes, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_2 + align_off, img2, img_bytes, hipMemcpyHostToDevice));
    if (H) HIPCHK(c, hipMemcpy(d_h, H, (size_t)n * 36, hipMemcpyHostToDevice));
    if (planes) {                                                           // sentinel everywhere: what the launch leaves of it is the border it must not touch
        HIPCHK(c, t.alloc(&d_p, (size_t)c->n_planes * plane));
        HIPCHK(c, hipMemsetAsync(d_p, 0xA5, (size_t)c->n_planes * plane * 4, c->stream));
    }
    HIPCHK(c, launch_prep(d_1 + align_off, d_2 + align_off, pix_fmt, H ? d_h : nullptr, k, d_o, n, c->stream, d_p, d_p ? plane : 0, d_p ? c->n_planes : 3, c->warp_exact));
    if (d_p) HIPCHK(c, launch_s3pad_to_f32_nhwc(d_p, plane, d_o, n, c->n_planes, c->stream));
    HIPCHK(c, launch_nhwc_to_nchw(d_o, d_t, n, 2, ho, wo, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, d_t, n_out * 4, hipMemcpyDeviceToHost));
    if (d_p) HIPCHK(c, hipMemcpy(planes, d_p, (size_t)c->n_planes * plane * 4, hipMemcpyDeviceToHost));
    return HNET_OK;
}

int hnet_debug_layer_output(hnet_ctx* c, int layer, int pair, float* out, size_t cap) {
    if (!c || !out || layer < 0 || layer >= 20 || pair < 0 || pair >= c->cfg.max_batch) return HNET_ERR_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    const size_t n = (size_t)c->act_c[layer] * c->act_h[layer] * c->act_w[layer];
    if (cap < n) return fail(c, HNET_ERR_INVALID_ARG, "buffer too small");
    DevTemps t;
    float* d_t = nullptr;
    HIPCHK(c, t.alloc(&d_t, n));
    if (c->fuse_b4 && layer == 13) {   // the fused kernel keeps block_4_0's output in LDS: recompute it unfused for inspection
        if (c->b4_in_stale) return fail(c, HNET_ERR_UNSUPPORTED, "layer 13 of a batch > 8: block 4 sampled its input in-kernel (inspect it on a context without HNET_VARIANT_WARP_FUSE)");
        uint16_t* tmp = nullptr;
        HIPCHK(c, t.alloc(&tmp, 3 * n));
        const float* xin = c->x_in[3] + (size_t)pair * NPIX * 2;
        if (c->x16_b4) {                 // the block-4 input only exists as padded bf16 planes: their sum is the exact fp32 value
            float* xf = nullptr;
            HIPCHK(c, t.alloc(&xf, (size_t)NPIX * 2));
            HIPCHK(c, launch_s3pad_to_f32_nhwc(c->x16_b4 + (size_t)pair * B4_HP * B4_WP, c->x16_plane, xf, 1, c->n_planes, c->stream));
            xin = xf;
        }
        HIPCHK(c, launch_conv(13, xin, 1, IMG_H, IMG_W, c->conv_w[13], c->conv_b[13], nullptr, c->stream,
                              nullptr, 0, tmp, n));
        HIPCHK(c, launch_nhwc_s3_to_nchw_f32(tmp, n, d_t, 1, c->act_c[13], c->act_h[13], c->act_w[13], c->stream));   // three planes: written by the fp32-MFMA kernel
    } else if (c->fuse_b42 && layer == 15) {   // block_4_2's output lives in LDS only: recompute it with the stand-alone patch kernel for inspection
        uint16_t* tmp = nullptr;
        HIPCHK(c, t.alloc(&tmp, 3 * n));
        const size_t n14 = c->act_count[14];
        const uint16_t* a14 = c->act16[14] + (size_t)pair * n14;
        size_t a14_plane = (size_t)c->cfg.max_batch * n14;
        if (c->a14_pad) {                          // bordered layout -> a plain copy of this pair
            uint16_t* plain = nullptr;
            HIPCHK(c, t.alloc(&plain, 2 * n14));
            HIPCHK(c, launch_s3_repitch(c->act16[14] + (size_t)pair * B42_IMG * 16, (size_t)c->cfg.max_batch * B42_IMG * 16, plain, n14, 1, c->act_h[14], c->act_w[14], 16,
                                        B42_HP, B42_WP, B42_PADY, B42_PADX, false, c->stream, 2));
            a14 = plain; a14_plane = n14;
        }
        HIPCHK(c, launch_conv_patch(15, a14, a14_plane, 1, c->act_h[14], c->act_w[14], c->patch_frag[15],
                                    c->conv_b[15], tmp, n, c->stream, c->n_planes, c->patch_b128, c->patch_rb5));
        HIPCHK(c, launch_nhwc_s3_to_nchw_f32(tmp, n, d_t, 1, c->act_c[15], c->act_h[15], c->act_w[15], c->stream, c->n_planes));
    } else if (c->fuse_b3 && layer == 7) {   // the fused block-3 kernel keeps block_3_0's output in LDS: recompute it unfused for inspection
        uint16_t* tmp = nullptr;
        HIPCHK(c, t.alloc(&tmp, 3 * n));
        HIPCHK(c, launch_conv_first_s3(c->x_in[2] + (size_t)pair * (NPIX / 4) * 2, c->b30_frag, c->conv_b[7], tmp, n, 1, IMG_H / 2, IMG_W / 2, c->stream, c->n_planes));
        HIPCHK(c, launch_nhwc_s3_to_nchw_f32(tmp, n, d_t, 1, c->act_c[7], c->act_h[7], c->act_w[7], c->stream, c->n_planes));
    } else if (layer == 14 && c->a14_pad) {        // bordered layout -> a plain copy of this pair
        uint16_t* plain = nullptr;
        HIPCHK(c, t.alloc(&plain, 2 * n));
        HIPCHK(c, launch_s3_repitch(c->act16[14] + (size_t)pair * B42_IMG * 16, (size_t)c->cfg.max_batch * B42_IMG * 16, plain, n, 1, c->act_h[14], c->act_w[14], 16,
                                    B42_HP, B42_WP, B42_PADY, B42_PADX, false, c->stream, 2));
        HIPCHK(c, launch_nhwc_s3_to_nchw_f32(plain, n, d_t, 1, c->act_c[layer], c->act_h[layer], c->act_w[layer], c->stream, 2));
    } else if (c->act16[layer])
        HIPCHK(c, launch_nhwc_s3_to_nchw_f32(c->act16[layer] + (size_t)pair * n, (size_t)c->cfg.max_batch * n, d_t, 1, c->act_c[layer],
                                             c->act_h[layer], c->act_w[layer], c->stream,
                                             (conv_is_first_s2(layer) && !c->first_s2) ? 3 : c->n_planes));   // HNET_FIRST_S2=0: block_1_1 / block_2_1 from the fp32-MFMA kernel, three planes
    else
        HIPCHK(c, launch_nhwc_to_nchw(c->act[layer] + (size_t)pair * n, d_t, 1, c->act_c[layer], c->act_h[layer], c->act_w[layer], c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, d_t, n * 4, hipMemcpyDeviceToHost));
    return HNET_OK;
}

int hnet_debug_h_part1(hnet_ctx* c, int pair, float* out9) {
    if (!c || !out9 || pair < 0 || pair >= c->cfg.max_batch) return HNET_ERR_INVALID_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out9, (c->H_last ? c->H_last : c->Hm) + (size_t)pair * 9, 36, hipMemcpyDeviceToHost));
    return HNET_OK;
}

int hnet_infer_batch_seqs_packed_device(hnet_ctx* c, const void* d_prev, const void* d_curr, int pix_fmt, const float* d_prior, int batch,
                                        const uint64_t* d_pair_seq, float* d_out72, float* d_err_map, void* stream) {
    hipStream_t s = nullptr;
    const int rc = device_entry(c, d_prev && d_curr && d_pair_seq && d_out72, pix_fmt, d_err_map, stream, s);
    return rc != HNET_OK ? rc : forward(c, FwdArgs{.prev = d_prev, .curr = d_curr, .pix_fmt = pix_fmt, .prior = d_prior, .batch = batch,
                                                   .mean = d_out72, .cov = d_out72 + 8, .err = d_err_map, .seq_tab = d_pair_seq,
                                                   .mean_stride = HNET_PACKED_FLOATS, .cov_stride = HNET_PACKED_FLOATS}, s);
}

}  // extern "C"
