// capi_forward.hip — one forward of the model as a fixed sequence of kernel launches on one stream (forward), and the list of those launches
// that the per-stage profile reports (build_stages).
#include "capi_internal.h"

// `make ROCTX=1` (-DHNET_ROCTX, links libroctx64): roctx ranges around the forward and around each block, visible in rocprofv3 --marker-trace and in
// the timeline tools - the counterpart of the stopwatches the reference brackets `forward` with (HomographyNet.cpp:178-188).  Off in the default build:
// the hot path makes no call into a tracing library.
#ifdef HNET_ROCTX
#include <roctracer/roctx.h>
struct HnetRange {
    explicit HnetRange(const char* name) { roctxRangePush(name); }
    ~HnetRange() { roctxRangePop(); }
    HnetRange(const HnetRange&) = delete;
};
#define HNET_RANGE(var, name) HnetRange var(name)
#else
#define HNET_RANGE(var, name) do { } while (0)
#endif

using namespace hnet;

namespace capi {

// block 4 of a forward of `batch` pairs samples its own input (no prep_b4 launch); prev == nullptr: images unknown yet - the usual case (4-byte aligned u8) is assumed
static bool b4_warp_in(const hnet_ctx* c, int batch, const void* prev, const void* curr, int pix_fmt) {
    if (!c->warp_in || !c->fuse_b4 || !c->x16_b4 || c->n_planes != 2 || (c->fuse_small && batch <= 8)) return false;
    return prev ? block4_warp_in_supported(prev, curr, pix_fmt == HNET_PIX_U8, c->n_planes) : true;
}

// the launches of one forward of `batch` pairs, in order (what the STAGE macro of forward_chunk records events for): the latency path
// (batch <= 8) has fewer of them
void build_stages(hnet_ctx* c, int batch, const void* prev, const void* curr, int pix_fmt) {      // (image pointers: forward_chunk fuses the block tail into a prep launch only for 16-byte-aligned images)
    c->stages.clear();
    const hnet_config& g = c->cfg;
    auto conv_flops = [&](int l, int h, int w) {
        const ConvDesc& d = kConvs[l];
        return 2.0 * d.cout * d.cin * d.ks * d.ks * conv_out_dim(h, d.ks, d.stride) * conv_out_dim(w, d.ks, d.stride);
    };
    static const int first[4] = {0, 3, 7, 13}, last[4] = {2, 6, 12, 19}, chain_first[4] = {1, 4, 10, 17};
    const bool small = c->fuse_small && batch <= 8;
    bool pend = false;
    if (g.use_prior) {
        if (small) pend = true;
        else c->stages.push_back({"prior_dlt", 0});
    }
    const int fb = g.use_prior ? 4 - g.blocks_to_run : 0;
    for (int blk = fb; blk < 4; blk++) {
        const bool fused_prep = pend && (prev ? prep_fc_supported(prev, curr, 8 >> blk, blk == 3 && c->x16_b4 != nullptr) : (blk < 3 || c->x16_b4 != nullptr));
        if (pend && !fused_prep) c->stages.push_back({blk == fb && g.use_prior ? "prior_dlt" : "fc_dlt_b" + std::to_string(blk), blk == fb && g.use_prior ? 0.0 : 2.0 * 8 * 5120});
        if (!(blk == 3 && !pend && b4_warp_in(c, batch, prev, curr, pix_fmt)))       // (block 4 of a large batch samples its input itself: conv_b4_fused.h WARPIN)
        c->stages.push_back({std::string(fused_prep ? (blk == fb && g.use_prior ? "prior_dlt+" : "fc_dlt+") : "") + "prep_b" + std::to_string(blk + 1),
                             fused_prep && !(blk == fb && g.use_prior) ? 2.0 * 8 * 5120 : 0.0});
        pend = false;
        int h = IMG_H >> (3 - blk), w = IMG_W >> (3 - blk);
        for (int l = first[blk]; l <= last[blk]; l++) {
            double fl = conv_flops(l, h, w);
            std::string nm = kConvs[l].name;
            h = conv_out_dim(h, kConvs[l].ks, kConvs[l].stride);
            w = conv_out_dim(w, kConvs[l].ks, kConvs[l].stride);
            if (c->fuse_b42 && l == 15) {      // one launch for block_4_2 + block_4_3
                fl += conv_flops(16, h, w);
                nm = "block_4_2+4_3";
                h = conv_out_dim(h, kConvs[16].ks, kConvs[16].stride);
                w = conv_out_dim(w, kConvs[16].ks, kConvs[16].stride);
                l = 16;
            }
            if (c->fuse_b3 && l == 7) {        // one launch for block_3_0 + block_3_1
                fl += conv_flops(8, h, w);
                nm = "block_3_0+3_1";
                h = conv_out_dim(h, kConvs[8].ks, kConvs[8].stride);
                w = conv_out_dim(w, kConvs[8].ks, kConvs[8].stride);
                l = 8;
            }
            if (c->use_chain && small && l == chain_first[blk]) {      // one launch for the block's tail (chain_lat.h)
                for (int l2 = l + 1; l2 <= last[blk]; l2++) {
                    fl += conv_flops(l2, h, w);
                    h = conv_out_dim(h, kConvs[l2].ks, kConvs[l2].stride);
                    w = conv_out_dim(w, kConvs[l2].ks, kConvs[l2].stride);
                    nm += std::string("+") + (kConvs[l2].name + 6);      // "block_4_4+4_5+4_6"
                }
                l = last[blk];
            }
            if (c->fuse_b4 && l == 13) {       // one launch for block_4_0 + block_4_1
                fl += conv_flops(14, h, w);
                nm = "block_4_0+4_1";
                h = conv_out_dim(h, kConvs[14].ks, kConvs[14].stride);
                w = conv_out_dim(w, kConvs[14].ks, kConvs[14].stride);
                l = 14;
            }
            c->stages.push_back({nm, fl});
        }
        if (blk < 3) {
            if (small) pend = true;
            else c->stages.push_back({"fc_dlt_b" + std::to_string(blk + 1), 2.0 * 8 * 5120});
        }
    }
    c->stages.push_back({"heads_fc1", 2.0 * 512 * 5120 * c->n_local});
    if (small && c->n_local <= HEADS_FC2_FINISH_MAX_N) c->stages.push_back({"heads_fc2+mc_finish", 2.0 * 16 * 256 * c->n_local});
    else {
        c->stages.push_back({"heads_fc2", 2.0 * 16 * 256 * c->n_local});
        c->stages.push_back({"mc_finish", 0});
    }
    if (g.emit_error_map) c->stages.push_back({"errmap", 0});
}

#define STAGE(call)                                                                                         \
    do {                                                                                                    \
        hipError_t e_ = (call);                                                                             \
        stage_i++;                                                                                          \
        if (e_ != hipSuccess) return fail(c, HNET_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); \
        if (!c->prof_ev.empty() && c->prof_pos < c->prof_ev.size()) {                                       \
            e_ = hipEventRecord(c->prof_ev[c->prof_pos++], s);                                              \
            if (e_ != hipSuccess) return fail(c, HNET_ERR_DEVICE, "hipEventRecord(stage)");                 \
        }                                                                                                   \
    } while (0)

// The forward of combined_stu_model (model_to_trace.py:299-330) for `a.batch` independent frame pairs that occupy
// slots [a.pair0, a.pair0 + a.batch) of the persistent buffers; everything is enqueued on stream `s`.
static int forward_chunk(hnet_ctx* c, const FwdArgs& a, hipStream_t s) {
    const hnet_config& g = c->cfg;
    const int B = a.batch;
    const size_t P0 = (size_t)a.pair0;
    static const int first[4] = {0, 3, 7, 13}, last[4] = {2, 6, 12, 19}, chain_first[4] = {1, 4, 10, 17};
    float* Hm = c->Hm + P0 * 9;
    float* Htot = c->Htot + P0 * 9;
    float* ws = c->ws;                             // split-K workspace
    const size_t wsn = c->ws_floats;
    // Latency path (batch <= 8): the homography of a block is not produced by a launch of its own (prior DLT / FC + DLT + composition) but
    // recomputed inside the next block's prep kernel by every workgroup (kernels.h FcArgs): 3-4 launches fewer in the dependent chain.
    // `pend` holds what the next prep has to evaluate; the homographies alternate between Hm and Hm2 (a workgroup stores the new one while
    // others still read the old one).
    const bool small = c->fuse_small && B <= 8;
    uint32_t* const flagp = a.flag ? a.flag : c->d_flag;
    size_t stage_i = 0;                            // launches so far (index into c->stages when that list describes this forward)
    auto set_kernels = [&](int k) { if (stage_i >= 1 && stage_i <= c->stages.size()) c->stages[stage_i - 1].kernels = k; };
    // the keep bits of the heads depend on the seeds only: on the latency path they are drawn by surplus workgroups of block 4's prep launch (FcArgs::mask)
    const bool mask_in_prep = small && c->lat_tail && c->s3 && heads_fc1_one_launch(B, c->n_local, c->n_planes);
    bool mask_ready = false;
    FcArgs pend = {};
    bool have_pend = false;
    float* Hcur = Hm;                              // buffer holding the homography so far
    float* Hnext = c->Hm2 + P0 * 9;
    if (g.use_prior) {
        if (small) { pend = FcArgs{nullptr, nullptr, nullptr, nullptr, a.prior, nullptr}; have_pend = true; }
        else STAGE(launch_prior_dlt(a.prior, Hm, B, s));                               // :129-130
    }
    const int fb = g.use_prior ? 4 - g.blocks_to_run : 0;
    HNET_RANGE(range_fwd, "hnet forward");
    for (int blk = fb; blk < 4; blk++) {
        static const char* const kBlockRange[4] = {"hnet block 1", "hnet block 2", "hnet block 3", "hnet block 4 trunk"};
        HNET_RANGE(range_blk, kBlockRange[blk]);
        (void)kBlockRange;
        const bool warp = g.use_prior || blk > 0;                                    // block 1 of the full model sees raw img2 (:138)
        int h = IMG_H >> (3 - blk), w = IMG_W >> (3 - blk);
        float* x = c->x_in[blk] + P0 * h * w * 2;
        const bool b4_dma = blk == 3 && c->x16_b4 != nullptr;      // block 4 always warps (:261): the prep kernel writes the padded planes
        uint32_t* x16 = b4_dma ? c->x16_b4 + P0 * B4_HP * B4_WP : nullptr;
        B4Warp b4w = {};
        bool b4w_on = false;
        if (blk == 3) c->b4_in_stale = false;
        if (have_pend) {
            if (prep_fc_supported(a.prev, a.curr, 8 >> blk, x16 != nullptr)) {
                pend.H_out = pend.feat ? Hnext : Hcur;                                // the prior's DLT has no input homography: it may land in Hcur
                if (blk == 3 && mask_in_prep) {
                    pend.mask = c->head_mask + P0 * c->n_local * 2 * 640;
                    pend.mask_blocks = (int)(((size_t)B * c->n_local * 2 * 160 + 255) / 256);
                    pend.n_local = c->n_local; pend.s_begin = c->s_begin; pend.thr = hnet_drop_threshold(g.dropout_p);
                    pend.mc_seed = g.mc_seed; pend.pair_seq0 = a.seq0; pend.seq_dev = a.seq_dev; pend.seq_tab = a.seq_tab;
                    mask_ready = true;
                }
                STAGE(launch_prep_fc(a.prev, a.curr, a.pix_fmt, pend, 8 >> blk, x, B, s, x16, c->x16_plane, c->n_planes, c->warp_exact));
                if (pend.feat) std::swap(Hcur, Hnext);
            } else {                                                                  // (unaligned images / K = 8: the separate launches)
                if (pend.feat) STAGE(launch_block_fc_dlt(pend.feat, pend.wfc, pend.bfc, pend.H_in, Hcur, B, s));
                else STAGE(launch_prior_dlt(pend.prior, Hcur, B, s));
                STAGE(launch_prep(a.prev, a.curr, a.pix_fmt, Hcur, 8 >> blk, x, B, s, x16, c->x16_plane, c->n_planes, c->warp_exact));
            }
            have_pend = false;
        } else if (blk == 3 && b4_warp_in(c, B, a.prev, a.curr, a.pix_fmt)) {
            b4w = B4Warp{(const uint8_t*)a.prev, (const uint8_t*)a.curr, Hcur};          // no launch: block_4_0 + block_4_1 samples cat(img1, warp(img2, H)) itself
            b4w_on = true;
            c->b4_in_stale = true;
        } else {
            STAGE(launch_prep(a.prev, a.curr, a.pix_fmt, warp ? Hcur : nullptr, 8 >> blk, x, B, s, x16, c->x16_plane, c->n_planes, c->warp_exact));
        }
        const float* in = x;
        const uint16_t* in16 = nullptr;
        size_t in_plane = 0;
        const size_t MB = (size_t)g.max_batch;
        bool chain_fc_done = false;                // this block's tail chain left the FC's partial sums in c->fc_part
        for (int l = first[blk]; l <= last[blk]; l++) {
            if (c->use_chain && small && P0 == 0 && l == chain_first[blk] && in16) {      // the block's tail in one launch on one XCD (chain_lat.h)
                int nxt = blk < 3 ? blk + 1 : fb;                                         // the chain launch that follows this one on the stream: the next block's, or the next forward's first
                if (nxt == blk) {                                                         // prior-1: ONE chain per forward - nobody else zeroes its area: a memset node in front of it
                    if (hipMemsetAsync(c->chain_sync + blk * CH_SYNC_WORDS, 0, CH_SYNC_WORDS * sizeof(uint32_t), s) != hipSuccess) return fail(c, HNET_ERR_DEVICE, "chain area memset");
                    nxt = 0;
                }
                ChainArgs cargs = c->chain_args[blk];
                cargs.flag = flagp;
                chain_fc_done = blk < 3 && cargs.fcw != nullptr;
                STAGE(launch_tail_chain(blk + 1, cargs, c->chain_sync + blk * CH_SYNC_WORDS, c->chain_sync + nxt * CH_SYNC_WORDS, B, s, c->chain_grid));
                l = last[blk];
                in = c->act[l];
                in16 = nullptr;
                in_plane = 0;
                h = c->act_h[l]; w = c->act_w[l];
                continue;
            }
            if (c->fuse_b4 && l == 13) {       // block_4_0 + block_4_1 in one launch; the 8-channel map stays in LDS
                const size_t cnt1 = c->a14_pad ? B42_IMG * 16 : c->act_count[14];
                uint16_t* o16 = c->act16[14] + P0 * cnt1;
                STAGE(launch_block4_fused(b4_dma ? (const void*)x16 : (const void*)in, c->x16_plane, c->b40_frag, c->conv_b[13], c->b41_frag, c->conv_b[14], o16,
                                          MB * cnt1, B, s, c->b4_flags | (c->a14_pad ? 64 : 0), c->n_planes, b4w_on ? &b4w : nullptr));
                in = nullptr; in16 = o16; in_plane = MB * cnt1;
                h = c->act_h[14]; w = c->act_w[14];
                l = 14;
                continue;
            }
            if (c->fuse_b42 && c->a14_pad && l == 15 && c->n_planes == 2 && c->b42_w2 && c->b42_w3 && in16 && h == 112 && w == 160) {   // block_4_2 + block_4_3 in one launch
                const size_t cnt1 = c->act_count[16];
                uint16_t* o16b = c->act16[16] + P0 * cnt1;
                STAGE(launch_block42_fused(in16, in_plane, c->b42_w2, c->conv_b[15], c->b42_w3, c->conv_b[16], o16b, MB * cnt1, B, s, c->n_planes));
                in = nullptr; in16 = o16b; in_plane = MB * cnt1;
                h = c->act_h[16]; w = c->act_w[16];
                l = 16;
                continue;
            }
            if (c->fuse_b3 && l == 7 && c->n_planes == 2 && c->b30_frag && c->b3f_w1 && h == 112 && w == 160) {   // block_3_0 + block_3_1 in one launch
                const size_t cnt1 = c->act_count[8];
                uint16_t* o16b = c->act16[8] + P0 * cnt1;
                STAGE(launch_block3_fused(in, c->b30_frag, c->conv_b[7], c->b3f_w1, c->conv_b[8], o16b, MB * cnt1, B, s, c->n_planes));
                in = nullptr; in16 = o16b; in_plane = MB * cnt1;
                h = c->act_h[8]; w = c->act_w[8];
                l = 8;
                continue;
            }
            const size_t cnt = c->act_count[l];
            float* o = c->act[l] ? c->act[l] + P0 * cnt : nullptr;
            uint16_t* o16 = c->act16[l] ? c->act16[l] + P0 * cnt : nullptr;
            if (c->s3 && l == 7 && c->b30_s3 && c->b30_frag && o16)
                STAGE(launch_conv_first_s3(in, c->b30_frag, c->conv_b[l], o16, MB * cnt, B, h, w, s, c->n_planes));
            else if (c->s3 && conv_is_first_s2(l) && c->first_s2 && c->s2_frag[l] && o16)
                STAGE(launch_conv_first_s2(l, in, c->s2_frag[l], c->conv_b[l], o16, MB * cnt, B, s, c->n_planes));
            else if (c->use_patch && (conv_is_patch_layer(l) || (c->use_patch32 && conv_is_patch32_layer(l) && h == 56 && w == 80)))
                STAGE(launch_conv_patch(l, in16, in_plane, B, h, w, c->patch_frag[l], c->conv_b[l], o16, MB * cnt, s, c->n_planes, c->patch_b128, c->patch_rb5));
            else if (c->s3 && conv_is_s3_layer(l)) {
                LatIO lat = {c->lat_tail && ws ? reinterpret_cast<uint32_t*>(c->ws + c->ws_floats) : nullptr, 1, false, false};
                STAGE(launch_conv_s3(l, in16, in_plane, B, h, w, c->conv_w16[l], (size_t)kConvs[l].cout * conv_padded_k(l),
                                     c->conv_b[l], o16, MB * cnt, o16 ? nullptr : o, s, ws, wsn, c->conv_wfrag[l], c->n_planes, c->s3_tile, &lat));
                set_kernels(lat.kernels);
            } else
                STAGE(launch_conv(l, in, B, h, w, c->conv_w[l], c->conv_b[l], o, s, ws, wsn, o16, MB * cnt));
            in = o;
            in16 = o16;
            in_plane = MB * cnt;
            h = c->act_h[l];
            w = c->act_w[l];
        }
        if (blk < 3) {                                                                // :143-150, :163-168, :183-188
            if (small) {
                pend = FcArgs{in, c->fc_w[blk], c->fc_b[blk], warp ? Hcur : nullptr, nullptr, nullptr};
                if (chain_fc_done) pend.fc_part = c->fc_part;      // (the unaligned-image fallback below still computes the FC from `in`)
                have_pend = true;
            }
            else STAGE(launch_block_fc_dlt(in, c->fc_w[blk], c->fc_b[blk], warp ? Hcur : nullptr, Hcur, B, s));
        }
    }
    Hm = Hcur;                                     // H_part1 of this forward
    c->H_last = Hcur - P0 * 9;
    // block 4 heads (:272-282) and output assembly (:310-317)
    HNET_RANGE(range_heads, "hnet heads + ensemble");
    const float* feat = c->act[19] + P0 * 5120;
    float* hidden = c->hidden + P0 * c->n_local * 512;
    if (c->s3) {
        LatIO lat_h = {nullptr, 1, small && c->lat_tail && c->n_planes == 2, mask_ready};
        STAGE(launch_heads_fc1_s3(feat, B, c->n_local, c->s_begin, g.dropout_p, g.mc_seed, a.seq0, c->w1_16, c->b1, hidden,
                                  c->feat16 + P0 * 5120, (size_t)g.max_batch * 5120, c->head_mask + P0 * c->n_local * 2 * 640, s, ws, wsn, a.seq_dev, c->n_planes,
                                  c->s3_tile, &lat_h, a.seq_tab, c->w1_feat_scale));
        set_kernels(lat_h.kernels);
    }
    else
        STAGE(launch_heads_fc1(feat, B, c->n_local, c->s_begin, g.dropout_p, g.mc_seed, a.seq0, c->w1, c->b1, hidden, s, ws, wsn, a.seq_dev, a.seq_tab));
    if (a.partial) {
        STAGE(launch_heads_fc2(hidden, B, c->n_local, c->s_begin, g.dropout_p, g.mc_seed, a.seq0, c->w2, c->b2,
                               a.mean_s, a.logvar_s, s, a.seq_dev, flagp, a.seq_tab));
        if (a.h_part1) {
            hipError_t e = hipMemcpyAsync(a.h_part1, Hm, (size_t)B * 9 * sizeof(float), hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) return fail(c, HNET_ERR_DEVICE, "copy H_part1");
        }
        return HNET_OK;
    }
    float* ms = c->mean_s + P0 * c->n_local * 8;
    float* lv = c->logvar_s + P0 * c->n_local * 8;
    if (small && c->n_local <= HEADS_FC2_FINISH_MAX_N) {
        STAGE(launch_heads_fc2_finish(hidden, B, c->n_local, c->s_begin, g.dropout_p, g.mc_seed, a.seq0, c->w2, c->b2, Hm, a.mean, a.cov, Htot, s,
                                      a.seq_dev, flagp, a.mean_stride, a.cov_stride, a.seq_tab));
    } else {
        STAGE(launch_heads_fc2(hidden, B, c->n_local, c->s_begin, g.dropout_p, g.mc_seed, a.seq0, c->w2, c->b2, ms, lv, s, a.seq_dev, nullptr, a.seq_tab));
        STAGE(launch_mc_finish(ms, lv, c->n_local, Hm, B, a.mean, a.cov, Htot, s, flagp, a.mean_stride, a.cov_stride));
    }
    if (g.emit_error_map && (a.err || a.err_u8))                                     // :319-327
        STAGE(launch_errmap(a.prev, a.curr, a.pix_fmt, Htot, a.err, a.err_u8, B, s));
    return HNET_OK;
}

// Validates and enqueues the forward of the whole batch on stream `s`.
// (Round 1 had an HNET_STREAMS switch that cut the batch into chunks on separate HIP streams.  It never gave a speed-up and
// the round-2 determinism test showed run-to-run differences of ~1e-3 px between concurrent chunks on the split-bf16 path
// (tools/dbg_streams.py; single-stream runs are bit-reproducible), so the chunked mode was removed rather than shipped.)
int forward(hnet_ctx* c, const FwdArgs& a, hipStream_t s) {
    const hnet_config& g = c->cfg;
    if (a.batch < 1) return fail(c, HNET_ERR_INVALID_ARG, "batch < 1");
    if (a.batch > g.max_batch) return fail(c, HNET_ERR_CAPACITY, "batch exceeds max_batch");
    if (g.use_prior && !a.prior) return fail(c, HNET_ERR_INVALID_ARG, "context uses a prior but none was given");
    c->last_batch = a.batch;
    const int rc = forward_chunk(c, a, s);
    // a forward that stopped part-way may leave split-K tile counters of the latency path non-zero (a launch that failed after its predecessors ran):
    // they are zeroed again behind whatever was enqueued, so the next forward starts from the state it assumes (kernels.h SPLITK_TICKETS)
    if (rc != HNET_OK && c->ws) (void)hipMemsetAsync(c->ws + c->ws_floats, 0, SPLITK_TICKETS * sizeof(uint32_t), s);
    if (rc != HNET_OK && c->chain_sync) (void)hipMemsetAsync(c->chain_sync, 0, CH_AREAS * CH_SYNC_WORDS * sizeof(uint32_t), s);      // (likewise the chains' counter areas)
    return rc;
}

}  // namespace capi
