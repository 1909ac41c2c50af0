// capi_weights.hip — the HNETW001 weight blob and the device layouts of its weights (the kernels' plane and fragment formats).
#include "capi_internal.h"

using namespace hnet;

namespace capi {

bool parse_blob(const uint8_t* p, size_t len, Blob& out) {
    if (len < 12 || memcmp(p, "HNETW001", 8) != 0) return false;
    uint32_t n; memcpy(&n, p + 8, 4);
    if (n > 1024) return false;
    size_t pos = 12;
    struct Ent { std::string name; std::vector<uint32_t> dims; uint64_t off; size_t count; };
    std::vector<Ent> ents;
    for (uint32_t i = 0; i < n; i++) {
        if (pos + 4 > len) return false;
        uint32_t ln; memcpy(&ln, p + pos, 4); pos += 4;
        if (ln > 512 || pos + ln + 4 > len) return false;
        Ent e; e.name.assign((const char*)p + pos, ln); pos += ln;
        uint32_t nd; memcpy(&nd, p + pos, 4); pos += 4;
        if (nd > 8 || pos + 4 * nd + 8 > len) return false;
        e.count = 1;
        for (uint32_t d = 0; d < nd; d++) {
            uint32_t v; memcpy(&v, p + pos, 4); pos += 4;
            e.dims.push_back(v);
            if (v != 0 && e.count > (len / 4) / v) return false;     // the product cannot exceed the file (no 64-bit wrap)
            e.count *= v;
        }
        memcpy(&e.off, p + pos, 8); pos += 8;
        if (e.off % 4) return false;
        ents.push_back(e);
    }
    const size_t data0 = (pos + 63) / 64 * 64;
    if (data0 > len) return false;
    const size_t room = len - data0;                                  // bytes of the data section
    for (auto& e : ents) {                                            // offsets come from the file: every check without overflow
        if (e.off > room || e.count > (room - (size_t)e.off) / 4) return false;
        out.t.push_back({e.name, Tensor{e.dims, (const float*)(p + data0 + e.off), e.count}});
    }
    return true;
}

template <typename T>
static hipError_t upload(T** dst, const std::vector<T>& v) {
    hipError_t e = dalloc(dst, v.size());
    if (e != hipSuccess) return e;
    return hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

// conv weight [Cout][Cin][KS][KS] -> [Cout][KS][SPR*SEG], inner index r = kw*Cin + ci, zero padded (igemm.h)
static std::vector<float> pack_conv(const float* w, const ConvDesc& d, int kp) {
    const int rl = d.ks * d.cin, rlp = kp / d.ks;
    std::vector<float> out((size_t)d.cout * kp, 0.0f);
    for (int co = 0; co < d.cout; co++)
        for (int ci = 0; ci < d.cin; ci++)
            for (int kh = 0; kh < d.ks; kh++)
                for (int kw = 0; kw < d.ks; kw++) {
                    const int r = kw * d.cin + ci;
                    (void)rl;
                    out[(size_t)co * kp + kh * rlp + r] = w[(((size_t)co * d.cin + ci) * d.ks + kh) * d.ks + kw];
                }
    return out;
}

// 7x7 / Cin 2 / stride 1 first layers: B-operand fragments of the pixel-pair GEMM of conv_first.h.
// W'[kh][kk = 2*kw' + ci][(dx, co)] = W[co][ci][kh][kw' - dx]  (0 outside 0..6); fragment t of lane l:
//   Cout  8 (16x16x4): t = kh*4 + e,        n = l&15, g = l>>4, kk = 4g + e
//   Cout 16 (32x32x2): t = kh*8 + q*4 + e,  n = l&31, h = l>>5, kk = 8q + 4h + e
static std::vector<float> pack_first_weights(const float* w, int cout) {
    const int nfrag = cout == 8 ? 28 : 56;
    std::vector<float> out((size_t)nfrag * 64, 0.0f);
    for (int t = 0; t < nfrag; t++)
        for (int l = 0; l < 64; l++) {
            int kh, kk, n;
            if (cout == 8) { kh = t / 4; kk = 4 * (l >> 4) + (t % 4); n = l & 15; }
            else { kh = t / 8; const int q = (t % 8) / 4, e = t % 4; kk = 8 * q + 4 * (l >> 5) + e; n = l & 31; }
            const int kwp = kk >> 1, ci = kk & 1, dx = n / cout, co = n % cout, kw = kwp - dx;
            if (kw >= 0 && kw < 7) out[(size_t)t * 64 + l] = w[(((size_t)co * 2 + ci) * 7 + kh) * 7 + kw];
        }
    return out;
}

// linear weight [out][5120] with NCHW-flatten input index c*20+pix -> NHWC-flatten index pix*256+c
static std::vector<float> permute_fc(const float* w, int n_out) {
    std::vector<float> out((size_t)n_out * 5120);
    for (int o = 0; o < n_out; o++)
        for (int c = 0; c < 256; c++)
            for (int pix = 0; pix < 20; pix++) out[(size_t)o * 5120 + pix * 256 + c] = w[(size_t)o * 5120 + c * 20 + pix];
    return out;
}

// Weights -> device, in the layouts of the kernels of the context's arithmetic mode (c->s3, c->n_planes).  Called by hnet_create and again by
// demote_to_bf16x3 (buffers of an earlier call are released first).  On failure the caller destroys the context.
// weight planes of the implicit-GEMM layers (igemm_s3.h): the fp16 mode uses the two-plane activation split there (s3_wplanes_gemm)
static inline void wsplit_gemm(float w, int np, uint16_t& a, uint16_t& b, uint16_t& c3) {
    if (np == 2) { split2h(w, a, b); c3 = 0; }
    else split3(w, a, b, c3);
}
int upload_weights(hnet_ctx* c, const Blob& b) {
#define CK(expr)                                                                    \
    do {                                                                            \
        hipError_t e_ = (expr);                                                     \
        if (e_ != hipSuccess) {                                                     \
            fprintf(stderr, "hnet weights: %s: %s\n", #expr, hipGetErrorString(e_)); \
            return HNET_ERR_DEVICE;                                                 \
        }                                                                           \
    } while (0)
    {
        auto fr = [](auto*& p) { if (p) (void)hipFree(p); p = nullptr; };
        for (int l = 0; l < 20; l++) { fr(c->patch_frag[l]); fr(c->conv_w[l]); fr(c->conv_b[l]); fr(c->conv_w16[l]); fr(c->conv_wfrag[l]); fr(c->chain_w[l]); }
        for (int k = 0; k < 3; k++) { fr(c->fc_w[k]); fr(c->fc_b[k]); }
        fr(c->s2_frag[0]); fr(c->s2_frag[3]); fr(c->b30_frag); fr(c->b40_frag); fr(c->b41_frag); fr(c->w1_16); fr(c->b3f_w1); fr(c->b42_w2); fr(c->b42_w3);
        fr(c->w1); fr(c->b1); fr(c->w2); fr(c->b2);
    }
    // ---- weights: names are the reference state_dict keys (model_to_trace.py:88-115, :210-235)
    for (int l = 0; l < 20; l++) {
        const ConvDesc& d = kConvs[l];
        const std::string pre = std::string(d.block == 4 ? "model_last_block_list.0." : "model_part1.") + d.name + ".0.";
        const Tensor* w = b.find(pre + "weight", {(uint32_t)d.cout, (uint32_t)d.cin, (uint32_t)d.ks, (uint32_t)d.ks});
        const Tensor* bi = b.find(pre + "bias", {(uint32_t)d.cout});
        if (!w || !bi) return HNET_ERR_BAD_WEIGHTS;
        if (c->s3 && c->n_planes == 2 && chain_layer(l)) {      // latency path: the layer's weights as the fragments of its one-XCD tail chain (chain_lat.h)
            std::vector<uint16_t> fr;
            if (!chain_pack_weights(l, w->data, fr)) return HNET_ERR_BAD_WEIGHTS;
            CK(upload(&c->chain_w[l], fr));
        }
        if (c->s3 && l == 13) {     // block_4_0 for the fused kernel: K index 8g+j of step st = (kh = 2st + (g>>1), kk = 8(g&1) + j)
            std::vector<uint16_t> fr((size_t)5 * 3 * 64 * 8, 0);     // slot 4: kernel row 6 alone as 16x16x16 fragments (K = 4 gg + e = tap 2 gg + (e >> 1), ci = e & 1), low 8 bytes
            for (int ln = 0; ln < 64; ln++) {
                const int n = ln & 15, gg = ln >> 4, dx = n >> 3, co = n & 7;
                for (int e = 0; e < 4; e++) {
                    const int kk = 4 * gg + e, kw = (kk >> 1) - dx, ci = kk & 1;
                    if (kw < 0 || kw >= 7) continue;
                    uint16_t sp[3];
                    wsplit_np(w->data[(((size_t)co * 2 + ci) * 7 + 6) * 7 + kw], c->n_planes, sp[0], sp[1], sp[2]);
                    for (int pl = 0; pl < 3; pl++) fr[(((size_t)4 * 3 + pl) * 64 + ln) * 8 + e] = sp[pl];
                }
            }
            for (int st = 0; st < 4; st++)
                for (int ln = 0; ln < 64; ln++) {
                    const int n = ln & 15, gg = ln >> 4, kh = 2 * st + (gg >> 1);
                    if (kh >= 7) continue;
                    const int dx = n >> 3, co = n & 7;
                    for (int j = 0; j < 8; j++) {
                        const int kk = 8 * (gg & 1) + j, kw = (kk >> 1) - dx, ci = kk & 1;
                        if (kw < 0 || kw >= 7) continue;
                        uint16_t sp[3];
                        wsplit_np(w->data[(((size_t)co * 2 + ci) * 7 + kh) * 7 + kw], c->n_planes, sp[0], sp[1], sp[2]);
                        for (int pl = 0; pl < 3; pl++) fr[(((size_t)st * 3 + pl) * 64 + ln) * 8 + j] = sp[pl];
                    }
                }
            CK(upload(&c->b40_frag, fr));
        }
        if (c->s3 && l == 7) {      // block_3_0 for conv7_c2_s1_s3_kernel: lane (n = l&31 = (dx, co), hh = l>>5), kk = 8hh + j of kernel row kh
            std::vector<uint16_t> fr((size_t)7 * 3 * 64 * 8, 0);
            for (int kh = 0; kh < 7; kh++)
                for (int ln = 0; ln < 64; ln++) {
                    const int n = ln & 31, hh = ln >> 5, dx = n >> 4, co = n & 15;
                    for (int j = 0; j < 8; j++) {
                        const int kk = 8 * hh + j, kw = (kk >> 1) - dx, ci = kk & 1;
                        if (kw < 0 || kw >= 7) continue;
                        uint16_t sp[3];
                        wsplit_np(w->data[(((size_t)co * 2 + ci) * 7 + kh) * 7 + kw], c->n_planes, sp[0], sp[1], sp[2]);
                        for (int pl = 0; pl < 3; pl++) fr[(((size_t)kh * 3 + pl) * 64 + ln) * 8 + j] = sp[pl];
                    }
                }
            CK(upload(&c->b30_frag, fr));
            c->b30_s3 = true;
        }
        if (c->s3 && l == 8 && c->n_planes == 2) {   // block_3_1 for the fused kernel: lane (i, g) of n-tile nt, step st: channel 16 nt + i, tap 2 st + (g >> 1), ci 8 (g & 1) + j
            std::vector<uint16_t> f2((size_t)2 * 13 * 2 * 64 * 8, 0);
            for (int nt = 0; nt < 2; nt++)
                for (int st = 0; st < 13; st++)
                    for (int ln = 0; ln < 64; ln++) {
                        const int co = 16 * nt + (ln & 15), gg = ln >> 4, t = 2 * st + (gg >> 1);
                        if (t >= 25) continue;
                        const int kh = t / 5, kw = t % 5;
                        for (int j = 0; j < 8; j++) {
                            const int ci = 8 * (gg & 1) + j;
                            uint16_t a0, a1;
                            split2h(w->data[(((size_t)co * 16 + ci) * 5 + kh) * 5 + kw], a0, a1);
                            f2[((((size_t)nt * 13 + st) * 2 + 0) * 64 + ln) * 8 + j] = a0;
                            f2[((((size_t)nt * 13 + st) * 2 + 1) * 64 + ln) * 8 + j] = a1;
                        }
                    }
            CK(upload(&c->b3f_w1, f2));
        }
        if (c->s3 && (l == 15 || l == 16) && c->n_planes == 2) {   // block_4_2 / block_4_3 for the fused kernel (conv_b42_fused.h), two weight planes
            const int nnt = d.cout / 16, nst = l == 15 ? 5 : 9;
            std::vector<uint16_t> f2((size_t)nnt * nst * 2 * 64 * 8, 0);
            for (int nt = 0; nt < nnt; nt++)
                for (int st = 0; st < nst; st++)
                    for (int ln = 0; ln < 64; ln++) {
                        const int co = 16 * nt + (ln & 15), gg = ln >> 4;
                        const int t = l == 15 ? 2 * st + (gg >> 1) : st;           // 16 -> 32: two taps per 32-deep step; 32 -> 64: one
                        if (t >= 9) continue;
                        const int kh = t / 3, kw = t % 3;
                        for (int j = 0; j < 8; j++) {
                            const int ci = l == 15 ? 8 * (gg & 1) + j : 8 * gg + j;
                            uint16_t a0, a1;
                            split2h(w->data[(((size_t)co * d.cin + ci) * 3 + kh) * 3 + kw], a0, a1);
                            f2[((((size_t)nt * nst + st) * 2 + 0) * 64 + ln) * 8 + j] = a0;
                            f2[((((size_t)nt * nst + st) * 2 + 1) * 64 + ln) * 8 + j] = a1;
                        }
                    }
            CK(upload(l == 15 ? &c->b42_w2 : &c->b42_w3, f2));
        }
        if (c->s3 && conv_is_first_s2(l)) {   // lane (i = channel of the n-tile, g): kernel row 2 st + (g>>1), taps 4 (g&1) + (j>>1), ci = j&1
            const int nt_n = d.cout / 16;
            std::vector<uint16_t> fr((size_t)nt_n * 4 * 3 * 64 * 8, 0);
            for (int nt = 0; nt < nt_n; nt++)
                for (int st = 0; st < 4; st++)
                    for (int ln = 0; ln < 64; ln++) {
                        const int co = nt * 16 + (ln & 15), gg = ln >> 4, kh = 2 * st + (gg >> 1);
                        if (kh >= 7) continue;
                        for (int j = 0; j < 8; j++) {
                            const int kw = 4 * (gg & 1) + (j >> 1), ci = j & 1;
                            if (kw >= 7) continue;
                            uint16_t sp[3];
                            wsplit_np(w->data[(((size_t)co * 2 + ci) * 7 + kh) * 7 + kw], c->n_planes, sp[0], sp[1], sp[2]);
                            for (int pl = 0; pl < 3; pl++) fr[((((size_t)nt * 4 + st) * 3 + pl) * 64 + ln) * 8 + j] = sp[pl];
                        }
                    }
            CK(upload(&c->s2_frag[l], fr));
            c->first_s2 = true;
        }
        if (c->s3 && conv_is_patch32_layer(l)) {   // 32 -> 64, 3x3: step st = tap st; lane group g -> channels 8g .. 8g+7 (odd groups rotated by 4)
            std::vector<uint16_t> fr((size_t)4 * 9 * 3 * 64 * 8, 0);
            for (int nt = 0; nt < 4; nt++)
                for (int st = 0; st < 9; st++)
                    for (int ln = 0; ln < 64; ln++) {
                        const int n = nt * 16 + (ln & 15), gg = ln >> 4, kh = st / 3, kw = st % 3;
                        for (int j = 0; j < 8; j++) {
                            const int ci = 8 * gg + j;
                            uint16_t sp[3];
                            wsplit_np(w->data[(((size_t)n * 32 + ci) * 3 + kh) * 3 + kw], c->n_planes, sp[0], sp[1], sp[2]);
                            for (int pl = 0; pl < 3; pl++) fr[((((size_t)nt * 9 + st) * 3 + pl) * 64 + ln) * 8 + j] = sp[pl];
                        }
                    }
            CK(upload(&c->patch_frag[l], fr));
        }
        if (c->s3 && conv_is_patch_layer(l)) {   // 16 -> 32, KSxKS: step st = taps 2st, 2st+1; lane group g -> tap 2st + (g>>1), ci 8(g&1)+j
            const int ks = d.ks, nstep = (ks * ks + 1) / 2;
            std::vector<uint16_t> fr((size_t)2 * nstep * 3 * 64 * 8, 0);
            for (int nt = 0; nt < 2; nt++)
                for (int st = 0; st < nstep; st++)
                    for (int ln = 0; ln < 64; ln++) {
                        const int n = nt * 16 + (ln & 15), gg = ln >> 4, t = 2 * st + (gg >> 1);
                        if (t >= ks * ks) continue;
                        const int kh = t / ks, kw = t % ks;
                        for (int j = 0; j < 8; j++) {
                            // odd lane groups read their 16-byte chunk high half first (conv_patch_s2.h): element j = channel (j + 4) % 8 of the half
                            const int ci = 8 * (gg & 1) + (((gg & 1) && !c->patch_b128) ? (j + 4) % 8 : j);
                            uint16_t sp[3];
                            wsplit_np(w->data[(((size_t)n * 16 + ci) * ks + kh) * ks + kw], c->n_planes, sp[0], sp[1], sp[2]);
                            for (int pl = 0; pl < 3; pl++) fr[((((size_t)nt * nstep + st) * 3 + pl) * 64 + ln) * 8 + j] = sp[pl];
                        }
                    }
            CK(upload(&c->patch_frag[l], fr));
        }
        if (conv_is_first_direct(l)) CK(upload(&c->conv_w[l], pack_first_weights(w->data, d.cout)));
        else {
            const std::vector<float> packed = pack_conv(w->data, d, conv_padded_k(l));
            CK(upload(&c->conv_w[l], packed));
            if (c->s3 && l == 14) {                 // block_4_1 B-fragments for the fused kernel: tap t = 4*st + g, 8 channels
                std::vector<uint16_t> fr((size_t)7 * 3 * 64 * 8, 0);
                for (int st = 0; st < 7; st++)
                    for (int ln = 0; ln < 64; ln++) {
                        // fp16-plane mode: the tap table of kernels.h (lane-group pairs share one ds_read_b128), channels in order
                        const int n = ln & 15, gg = ln >> 4, t = c->n_planes == 2 ? b41_tap(st, gg) : 4 * st + gg;
                        if (t < 0 || t >= 25) continue;
                        const int kh = t / 5, kw = t % 5;
                        for (int j = 0; j < 8; j++) {
                            // three-plane / bf16 modes: odd lane groups read their 16-byte chunk high half first (conv_b4_fused.h): element j = channel (j + 4) % 8
                            const int ci = (c->n_planes != 2 && (gg & 1)) ? (j + 4) % 8 : j;
                            uint16_t sp[3];
                            wsplit_np(w->data[(((size_t)n * 8 + ci) * 5 + kh) * 5 + kw], c->n_planes, sp[0], sp[1], sp[2]);
                            for (int pl = 0; pl < 3; pl++) fr[(((size_t)st * 3 + pl) * 64 + ln) * 8 + j] = sp[pl];
                        }
                    }
                CK(upload(&c->b41_frag, fr));
            }
            if (c->s3 && conv_is_s3_layer(l)) {     // exact 3-way bf16 split of every weight: planes [3][Cout][Kp]
                std::vector<uint16_t> pl(packed.size() * 3);
                for (size_t i = 0; i < packed.size(); i++)
                    wsplit_gemm(packed[i], c->n_planes, pl[i], pl[packed.size() + i], pl[2 * packed.size() + i]);
                CK(upload(&c->conv_w16[l], pl));
            }
            if (c->n_planes == 2 && conv_region_layer(l)) {
                // igemm_region.h: the two weight planes as MFMA fragments in the order the kernel consumes them:
                // [Cout / 16][Cin / 64 chunks][taps, padded][2 steps][2 planes][64 lanes][8 halves]; lane (r = lane & 15, g = lane >> 4) holds
                // output channel 16 nt + r, input channels 64 c + 32 st + 8 g .. + 7 of tap t (taps >= KS x KS: the zero-weight padding tap of the K-split form)
                const int ntap = d.ks * d.ks, ntap_pad = conv_region_taps_padded(l), nchunk = d.cin / 64;
                std::vector<uint16_t> fr((size_t)(d.cout / 16) * nchunk * ntap_pad * 2 * 2 * 64 * 8, 0);
                for (int nt = 0; nt < d.cout / 16; nt++)
                    for (int cc = 0; cc < nchunk; cc++)
                        for (int t = 0; t < ntap; t++)
                            for (int st = 0; st < 2; st++)
                                for (int ln = 0; ln < 64; ln++)
                                    for (int e = 0; e < 8; e++) {
                                        const int n = nt * 16 + (ln & 15), ci = 64 * cc + 32 * st + 8 * (ln >> 4) + e;
                                        uint16_t sp[3];
                                        wsplit_gemm(w->data[(((size_t)n * d.cin + ci) * d.ks + t / d.ks) * d.ks + t % d.ks], 2, sp[0], sp[1], sp[2]);
                                        const size_t base = ((((size_t)(nt * nchunk + cc) * ntap_pad + t) * 2 + st) * 2) * 64 * 8;
                                        fr[base + (size_t)ln * 8 + e] = sp[0];
                                        fr[base + 64 * 8 + (size_t)ln * 8 + e] = sp[1];
                                    }
                CK(upload(&c->conv_wfrag[l], fr));
            }
        }
        CK(upload(&c->conv_b[l], std::vector<float>(bi->data, bi->data + d.cout)));
    }
    for (int k = 0; k < 3; k++) {
        const std::string pre = "model_part1.fc_block_" + std::to_string(k + 1) + ".";
        const Tensor* w = b.find(pre + "weight", {8, 5120});
        const Tensor* bi = b.find(pre + "bias", {8});
        if (!w || !bi) return HNET_ERR_BAD_WEIGHTS;
        CK(upload(&c->fc_w[k], permute_fc(w->data, 8)));
        CK(upload(&c->fc_b[k], std::vector<float>(bi->data, bi->data + 8)));
    }
    {
        static const char* heads[2] = {"fc_block_4_mean", "fc_block_4_uncertainty"};
        std::vector<float> w1, b1, w2, b2;
        for (int h = 0; h < 2; h++) {
            const std::string pre = std::string("model_last_block_list.0.") + heads[h] + ".";
            const Tensor* tw1 = b.find(pre + "1.weight", {256, 5120});
            const Tensor* tb1 = b.find(pre + "1.bias", {256});
            const Tensor* tw2 = b.find(pre + "4.weight", {8, 256});
            const Tensor* tb2 = b.find(pre + "4.bias", {8});
            if (!tw1 || !tb1 || !tw2 || !tb2) return HNET_ERR_BAD_WEIGHTS;
            std::vector<float> p = permute_fc(tw1->data, 256);
            w1.insert(w1.end(), p.begin(), p.end());
            b1.insert(b1.end(), tb1->data, tb1->data + 256);
            w2.insert(w2.end(), tw2->data, tw2->data + 8 * 256);
            b2.insert(b2.end(), tb2->data, tb2->data + 8);
        }
        CK(upload(&c->w1, w1)); CK(upload(&c->b1, b1)); CK(upload(&c->w2, w2)); CK(upload(&c->b2, b2));
        c->w1_feat_scale = 1.0f;
        if (c->s3) {
            // fp16 planes carry a value to 2^-37 ABSOLUTE (s3_format.h): head weights below 2^-15 - a network whose features are large, the heads scaled back -
            // lose relative precision, and features of 24 000 turn that into 1e-4 px (tests/test_gpu_f16x2_kernel_range.py).  Such a file gets its planes from
            // w 2^e, the largest weight in [2^-7, 2^-6) like PyTorch's default initialisation, and the feature is multiplied by 2^-e before ITS split
            // (launch_heads_fc1_s3 feat_scale; both exact).  Ordinary files: e = 0, the same planes as ever.
            int e = 0;
            if (c->n_planes == 2) {
                float m = 0.f;
                for (float v : w1) m = std::max(m, std::fabs(v));
                if (m > 0.f && m < 0x1p-15f) e = std::min(-7 - std::ilogb(m), 24);
            }
            const float up = std::ldexp(1.0f, e);
            c->w1_feat_scale = std::ldexp(1.0f, -e);
            std::vector<uint16_t> pl(w1.size() * 3);
            for (size_t i = 0; i < w1.size(); i++) wsplit_gemm(w1[i] * up, c->n_planes, pl[i], pl[w1.size() + i], pl[2 * w1.size() + i]);
            CK(upload(&c->w1_16, pl));
        }
    }

    return HNET_OK;
#undef CK
}

}  // namespace capi
