// capi_internal.h — what the host translation units of libhnet_hip.so share: the context, the forward's argument block and the functions
// that more than one of them calls.  hnet_capi.hip: contexts, images, the inference entry points and their repair policy, groups, operator and
// debug entry points; capi_weights.hip: the HNETW001 blob and the weight layouts; capi_forward.hip: the launch sequence of one forward;
// capi_sessions.hip: hnet_sessions_*; capi_filters.hip: hnet_filters_* (what it reads of the sessions: sessions_internal.h).  Nothing here is part of the C ABI.
#pragma once
#include "../../include/hnet.h"
#include "../../include/hnet_rng.h"
#include "geom.h"
#include "kernels.h"
#include "filters_dev.h"
#include "photo_dev.h"
#include "photo_align_dev.h"
#include "photo_pyramid_dev.h"
#include "photo_robust_dev.h"
#include "chain_args.h"
#include "s3_format.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

// internal to the library: hidden from its dynamic symbol table
namespace capi __attribute__((visibility("hidden"))) {

struct Tensor { std::vector<uint32_t> dims; const float* data; size_t count; };

struct Blob {
    std::vector<std::pair<std::string, Tensor>> t;
    // the tensor must have exactly the reference's shape (state_dict of model_to_trace.py:88-115, :210-235), not just its size
    const Tensor* find(const std::string& n, std::initializer_list<uint32_t> shape) const {
        for (auto& e : t)
            if (e.first == n) return e.second.dims == std::vector<uint32_t>(shape) ? &e.second : nullptr;
        return nullptr;
    }
};

// what one forward reads and writes; call sites set the fields they need by name
struct FwdArgs {
    const void *prev = nullptr, *curr = nullptr;
    int pix_fmt = HNET_PIX_U8;
    const float* prior = nullptr;
    int batch = 0;
    uint64_t seq0 = 0;
    float *mean = nullptr, *cov = nullptr;      // device outputs (finish path)
    float* err = nullptr;                       // device error map (float) or null
    uint8_t* err_u8 = nullptr;
    float *mean_s = nullptr, *logvar_s = nullptr, *h_part1 = nullptr;   // partial path outputs (device) or null
    bool partial = false;
    int pair0 = 0;            // first pair of this chunk inside the persistent buffers (caller arrays are pre-offset)
    const uint64_t* seq_dev = nullptr;   // device addend to seq0 (graph replays)
    const uint64_t* seq_tab = nullptr;   // device [batch]: the sequence number of every pair (replaces seq0 / seq_dev; hnet_sessions_infer, hnet_infer_batch_seqs_packed_device)
    int mean_stride = 8, cov_stride = 64;   // floats between consecutive pairs of `mean` / `cov` (72 / 72: the packed [B][72] record)
    uint32_t* flag = nullptr;               // where the kernels raise the overflow / timeout bits (nullptr: the context's device word; hnet_infer's graph: a word of its pinned block)
};
struct Stage { std::string name; double flops_per_pair; int kernels = 1; };      // kernels: what the launch of the last forward consisted of (hnet_stage_kernels)

}  // namespace capi

struct hnet_ctx {
    hnet_config cfg;
    hipStream_t stream = nullptr;
    std::string err;
    bool owns_stream = true;           // false: a member of an hnet_group (the group owns the streams)
    std::vector<uint8_t> blob_copy;    // HNET_PREC_F16X2 only: the weight blob, kept so that an activation overflow can demote the context to HNET_PREC_BF16X3
    // weights (device)
    float* conv_w[20] = {};
    float* conv_b[20] = {};
    float* fc_w[3] = {};
    float* fc_b[3] = {};
    float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;
    // activations (device), sized for cfg.max_batch
    // matrix-core modes (every precision but HNET_PREC_FP32): activations of the layers feeding a conv are 16-bit planes (s3_format.h)
    bool s3 = false;
    uint16_t* conv_w16[20] = {};       // [3][Cout][Kp] 16-bit weight planes of the Cin >= 8 layers (fp16 in HNET_PREC_F16X2, bf16 in the bf16 modes; s3_format.h)
    uint16_t* conv_wfrag[20] = {};     // fp16-plane mode, igemm_region.h layers (block_1_2, block_1_3, block_2_4 / 3_5 / 4_6): the weights as MFMA fragments in consumption order
    uint16_t* act16[20] = {};          // [planes][max_batch][Ho][Wo][Cout] 16-bit activation planes: two fp16 planes in the default mode, three / one bf16 planes in HNET_PREC_BF16X3 / _BF16
    bool fuse_b4 = false;              // block_4_0 + block_4_1 in one kernel (conv_b4_fused.h), every matrix-core mode
    int b4_flags = 0;                  // bit 0: the fused kernel walks its tiles from the end of the batch (hnet_op_block4_fused `reverse`, tests)
    uint32_t* x16_b4 = nullptr;        // block-4 input as padded 16-bit planes (fp16 / bf16 by mode) [planes][max_batch][B4_HP][B4_WP] dwords (DMA-staged fused kernel, kernels.h)
    size_t x16_plane = 0;              // dwords per plane
    int n_planes = 3;                  // 16-bit planes the matrix-core layers read and write = their arithmetic mode: 3 = split-bf16 (fp32-grade), 1 = plain bf16 (HNET_PREC_BF16), 2 = fp16 planes (HNET_PREC_F16X2, fp32-grade)
    uint16_t* patch_frag[20] = {};     // conv_patch_s2.h weight fragments of block_3_1 / block_4_2: [2][NSTEP][3][64] x 16 B
    bool use_patch = false;
    int patch_rb5 = 5;                 // HNET_PATCH_RB5: region rows per batch of staging loads in the 5x5 patch kernel (1 / 2 / as many as fit: 5 in the fp16 mode, 3 in split-bf16)
    int s3_tile = 0;                   // HNET_S3_TILE: tile-shape experiments of the implicit-GEMM layers (s3_dispatch.h), 0 = measured defaults
    bool patch_b128 = true;            // block_3_1 / block_4_2 read their fragments with ds_read_b128 from the interleaved layout (HNET_PATCH_B128=0: two ds_read_b64, half-major layout)
    bool fuse_b3 = false;              // block_3_0 + block_3_1 in one kernel (conv_b3_fused.h): fp16-plane mode, HNET_FUSE_B3=0 switches back
    // its weights: block_3_0 as the three-plane fragments b30_frag of conv_first.h, block_3_1 as [2][13][2][64] x 16 B
    uint16_t* b3f_w1 = nullptr;
    bool a14_pad = false;              // block_4_1's output (act16[14]) in the bordered layout of kernels.h B42_* (fused block-4 kernel -> LDS-DMA of the fused block_4_2 + 4_3 kernel)
    bool fuse_b42 = false;             // block_4_2 + block_4_3 in one kernel (conv_b42_fused.h): fp16-plane mode, HNET_FUSE_B42=0 switches back
    uint16_t* b42_w2 = nullptr;        // its weights: [2][5][2][64] x 16 B and [4][9][2][64] x 16 B fragments
    uint16_t* b42_w3 = nullptr;
    bool fuse_small = true;            // batch <= 8 (latency path): block-tail FC + DLT inside the next block's prep kernel, heads_fc2 + mc_finish in one launch (HNET_FUSE_SMALL=0: the separate launches; bit-identical)
    float* Hm2 = nullptr;              // second homography buffer of that path (a prep workgroup stores H while others still read the previous one)
    const float* H_last = nullptr;     // where the last forward left H_part1 (Hm or Hm2)
    bool warp_exact = false;           // HNET_WARP_EXACT=1: the prep kernels keep grid_sample's sampling positions bit for bit (kernels.hip, A/B switch); default: the fast sampler
    bool use_patch32 = true;           // block_3_2 / block_4_3 through conv_patch32_s2_kernel (HNET_PATCH32=0: implicit GEMM)
    uint16_t* b30_frag = nullptr;      // block_3_0 weights as 32x32x16 fragments of the pixel-pair GEMM [7][3][64] x 16 B (conv_first.h)
    bool b30_s3 = true;
    uint16_t* s2_frag[4] = {};         // block_1_1 / block_2_1 (layers 0, 3) weights as 16x16x32 A-fragments [Cout/16][4][3][64] x 16 B (conv7_c2_s2_s3_kernel)
    bool first_s2 = true;              // HNET_FIRST_S2=0: the round-1 fp32-MFMA implicit GEMM for these two layers
    uint16_t* b40_frag = nullptr;      // block_4_0 weights as 16x16x32 B-fragments of the pixel-pair GEMM [4][3][64] x 16 B, + slot [4]: kernel row 6 as 16x16x16 fragments
    uint16_t* b41_frag = nullptr;      // block_4_1 weights as 16x16x32 B-fragments [7][3][64] x 16 B
    uint16_t* w1_16 = nullptr;         // heads Linear(5120,256) x2: [3][512][5120] 16-bit weight planes (fp16 / bf16 by mode)
    float w1_feat_scale = 1.0f;        // fp16-plane mode, tiny head weights: w1_16 holds w / w1_feat_scale (a power of two), the feature is multiplied by it before its split (upload_weights)
    uint16_t* feat16 = nullptr;        // [planes][max_batch][5120] 16-bit planes: feat * 1/(1-p), split
    uint8_t* head_mask = nullptr;      // [max_batch][n_local][2][640] keep bits
    size_t act_count[20] = {};         // elements per pair of layer l's output
    float* x_in[4] = {};
    float* act[20] = {};
    int act_c[20], act_h[20], act_w[20];
    float* ws = nullptr;               // split-K partial sums (igemm.h), 64 MB, followed by the SPLITK_TICKETS tile counters of the latency path (kernels.h LatIO)
    size_t ws_floats = 0;
    // round 6: the tail of every block (its last 2 - 3 stride-2 layers) of a batch <= 8 as ONE launch on one XCD (chain_lat.h); fp16-plane mode, variant bit NO_CHAIN = off
    bool use_chain = false;
    float* fc_part = nullptr;          // [CH_MAX_PAIRS][32][8]: the block-tail FC as partial sums per item of a tail chain's last layer (chain_lat.h), read by the next warp + pool launch
    bool b4_in_stale = false;          // the last forward's block 4 sampled its input in-kernel: x16_b4 does not hold it (hnet_debug_layer_output(13) refuses)
    bool warp_in = false;              // batch > 8: block 4's warp + concat sampled inside the block_4_0 + block_4_1 kernel (conv_b4_fused.h WARPIN) - no prep_b4 launch
    int chain_grid = 256;              // workgroups of a chain launch (one per CU; HNET_VARIANT_CHAIN_GRID_8 / _3: the tests' small grids)
    uint16_t* chain_w[20] = {};        // the chain layers' weights as MFMA fragments (chain_pack_weights)
    hnet::ChainArgs chain_args[4] = {};      // one argument block per block's chain (passed by value)
    uint32_t* chain_sync = nullptr;    // CH_AREAS counter areas of CH_SYNC_WORDS words (claims, per-pair item / done counters), one per block's chain: the area of a launch is zero
                                       // when it starts - every chain launch zeroes the area of the NEXT chain launch of the forward sequence (stream ordered)
    bool lat_tail = true;              // round 5: split-K tiles of the 4 x 5 layers finished by their last-arriving workgroup, heads FC1 of small batches as one launch (heads_lat.h); variant 30 = off
    float *hidden = nullptr, *Hm = nullptr, *Htot = nullptr, *mean_s = nullptr, *logvar_s = nullptr;
    float *d_mean = nullptr, *d_cov = nullptr, *d_err = nullptr, *d_prior = nullptr;
    uint8_t* d_err_u8 = nullptr;
    void *stage_prev = nullptr, *stage_curr = nullptr;    // batch staging for host-buffer entry points (f32 sized)
    uint8_t* ring[2] = {};                                 // streaming prev / curr
    float* und_map[2] = {};                                // undistortion maps (x, y), 224x320 floats each (hnet_set_camera)
    uint8_t* raw_dev = nullptr;                            // staging of one raw frame
    int raw_rows = 0, raw_cols = 0;
    int curr_slot = 0;
    int img_counter = 0;
    double latest_t = -1.0;
    hnet_ctx* img_src = nullptr;       // hnet_attach_images: frames, counters and the mask sequence number are read from this context (the IEKF's iterative model)
    int n_local = 0, s_begin = 0;
    // timing
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_align[2] = {nullptr, nullptr};          // around the launch sequence of the last photometric alignment (photo_align_run): events of its own,
    double photo_align_ms = 0.0;                          // so that the read-only calls leave ev0 / ev1 and every hnet_timing as they were
    uint8_t* pyr_scratch = nullptr;                       // levels 1 .. 3 of img1 [max_batch] | img2 [max_batch] of a coarse-to-fine alignment; allocated on first use
    hnet_timing timing = {};
    std::vector<capi::Stage> stages;
    std::vector<hipEvent_t> prof_ev;   // when non-empty: one event after every stage
    size_t prof_pos = 0;
    int last_batch = 0;
    // hipGraph replay of small-batch forwards (29-45 dependent launches: at batch 1 the host launch cost dominates).
    // The sequence number of the MC-dropout masks lives in device memory (d_seq) and is refreshed by a memcpy node
    // from a pinned host word, so one captured graph serves every call.
    bool graph_zero_copy = false;      // ... whose kernels read {sequence number, prior} from and write {mean, cov, error map, flag} to the pinned host block directly (no memcpy nodes)
    bool use_graph = false;            // hnet_infer replays the forward as one hipGraph (default on; HNET_GRAPH=0: eager launches)
    bool graph_timing = false;         // hnet_time_batch_device too (HNET_GRAPH=1 only: the bare device time is 3 % better eager)
    uint64_t* d_seq = nullptr;
    uint32_t* d_flag = nullptr;        // hnet_overflow_flag: bit 0 = a forward produced a non-finite output since the last poll
    struct Pinned { uint64_t seq; float prior[8]; float mean[8]; float cov[64]; uint32_t flag; uint8_t err[HNET_IMG_ROWS * HNET_IMG_COLS]; };
    Pinned* pinned = nullptr;
    uint8_t* pinned_img[2] = {nullptr, nullptr};         // host staging of the pushed frame, one per ring slot
    hipEvent_t ev_img[2] = {nullptr, nullptr};           // its upload has completed
    hipGraphExec_t g_infer[2] = {nullptr, nullptr};      // hnet_infer, one per ring orientation
    const float* g_infer_H[2] = {nullptr, nullptr};      // where that graph's forward leaves H_part1 (H_last is only written while a forward is ENQUEUED, i.e. at capture time)
    const float* g_batch_H = nullptr;
    struct GraphKey { const void *prev, *curr, *prior, *mean, *cov; int batch, fmt; bool operator==(const GraphKey& o) const {
        return prev == o.prev && curr == o.curr && prior == o.prior && mean == o.mean && cov == o.cov && batch == o.batch && fmt == o.fmt; } };
    GraphKey g_key = {};
    hipGraphExec_t g_batch = nullptr;                     // hnet_time_batch_device on resident buffers (last signature)
};

namespace capi __attribute__((visibility("hidden"))) {

inline int fail(hnet_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

#define HIPCHK(c, expr)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return fail((c), HNET_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));    \
    } while (0)

template <typename T>
hipError_t dalloc(T** p, size_t count) { return hipMalloc((void**)p, std::max<size_t>(count, 1) * sizeof(T)); }

// A non-finite output only means "activation beyond the fp16-plane range" when the inputs were finite: a NaN prior of a diverged filter or a
// NaN float image gives NaN outputs in every arithmetic (the reference's too) and must not cost the context its mode.  (v == nullptr: nothing to test)
template <typename T>
bool all_finite(const T* v, size_t n) {
    for (size_t i = 0; v && i < n; i++) if (!std::isfinite(v[i])) return false;
    return true;
}

// The sections of a scratch block, carved in order: take<T>(count) is the next section, count elements of T at a 256-byte boundary; `used`: the bytes
// taken so far (base null: only the size is wanted)
struct Carver {
    uint8_t* base;
    size_t used = 0;
    template <typename T = uint8_t>
    T* take(size_t count) {
        T* p = reinterpret_cast<T*>(base + used);
        used += (count * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};

// The owner of device and pinned host memory: its destructor frees what it handed out; a default-constructed one holds nothing.  As a local (DevTemps) it
// holds the temporaries of an operator-level entry point, freed on every return path (HIPCHK returns early); as a member, the buffers of an object
// that are sized once and live as long as it does (the keyframe store and its layers, keyframes_internal.h).
struct DevMem {
    std::vector<void*> ptrs, pinned;           // device / pinned host
    DevMem() = default;
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    template <typename T>
    hipError_t alloc(T** p, size_t count) {
        const hipError_t e = dalloc(p, count);
        if (e == hipSuccess) ptrs.push_back((void*)*p);
        return e;
    }
    template <typename T>
    hipError_t alloc_pinned(T** p, size_t count) {
        const hipError_t e = hipHostMalloc((void**)p, count * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess) pinned.push_back((void*)*p);
        return e;
    }
    // what `o` owns becomes this owner's (allocate into a local, adopt on success: a failure leaves the object as it was)
    void adopt(DevMem& o) {
        for (void* q : o.ptrs) ptrs.push_back(q);
        for (void* q : o.pinned) pinned.push_back(q);
        o.ptrs.clear();
        o.pinned.clear();
    }
    ~DevMem() {
        for (void* q : ptrs) (void)hipFree(q);
        for (void* q : pinned) (void)hipHostFree(q);
    }
};
using DevTemps = DevMem;

// levels 1 .. 3 of img1 [max_batch] | img2 [max_batch] of a coarse-to-fine alignment (hnet_ctx::pyr_scratch): allocated by the first call that needs them
inline int ensure_pyr_scratch(hnet_ctx* c) {
    const size_t pyr = (size_t)c->cfg.max_batch * hnet::PYR_BYTES;
    if (!c->pyr_scratch) HIPCHK(c, dalloc(&c->pyr_scratch, 2 * pyr));
    return HNET_OK;
}

bool parse_blob(const uint8_t* p, size_t len, Blob& out);                                  // capi_weights.hip
int upload_weights(hnet_ctx* c, const Blob& b);          // weights -> device in the layouts of the context's arithmetic mode
void build_stages(hnet_ctx* c, int batch, const void* prev = nullptr, const void* curr = nullptr, int pix_fmt = HNET_PIX_U8);   // capi_forward.hip
int forward(hnet_ctx* c, const FwdArgs& a, hipStream_t s);
void record_timing(hnet_timing& t, float dev_ms, double host_ms, int n_inferences, bool main_model);      // hnet_capi.hip
int run_host_call(hnet_ctx* const ctx[2], const std::function<int(uint32_t* flag)>& enqueue, const std::function<int()>& overflowed);
// ... for a call that runs forwards on one context
inline int run_host_call(hnet_ctx* c, const std::function<int(uint32_t& flag)>& enqueue, const std::function<bool()>& overflowed) {
    hnet_ctx* const ctx[2] = {c, nullptr};
    return run_host_call(ctx, [&](uint32_t* flag) { return enqueue(flag[0]); }, [&] { return overflowed() ? 0 : -1; });
}
// photometric alignment of n pairs resident on the device (capi_photo_align.hip), single-level (levels = 1) or coarse to fine: d_x0 [n][8] start
// offsets; the launch sequence on c->stream, ONE download of the records - out [n] the level-0 records, levels_out null or [n][levels] - and one
// synchronisation.  The caller has validated n, levels (1 .. 4) and opts (photo_align_check_opts) and enqueued its upload on c->stream.
int photo_align_check_opts(hnet_ctx* c, const hnet_photo_align_opts* opts, const char* who);
int photo_align_run(hnet_ctx* c, const uint8_t* d_img1, const uint8_t* d_img2, int n, const float* d_x0, const hnet_photo_align_opts& opts, int levels,
                    hnet_photo_align* out, hnet_photo_align* levels_out);
// the same for the gain / bias + Huber alignment: out [n] and levels_out (null or [n][levels]) are hnet_photo_robust records
int photo_robust_check_opts(hnet_ctx* c, const hnet_photo_robust_opts* opts, const char* who);
int photo_align_run(hnet_ctx* c, const uint8_t* d_img1, const uint8_t* d_img2, int n, const float* d_x0, const hnet_photo_robust_opts& opts, int levels,
                    hnet_photo_robust* out, hnet_photo_robust* levels_out);
// the robust form on the template pixels the masks d_mask1 [n][NPIX] admit; opts checked by photo_robust_check_opts
int photo_align_masked_run(hnet_ctx* c, const uint8_t* d_img1, const uint8_t* d_mask1, const uint8_t* d_img2, int n, const float* d_x0,
                           const hnet_photo_robust_opts& opts, int levels, hnet_photo_robust* out, hnet_photo_robust* levels_out);
void build_undistort_maps(const hnet_camera* cam, std::vector<float>& mx, std::vector<float>& my);

}  // namespace capi
