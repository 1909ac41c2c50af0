// kernels_filters_keyframe.hip — the device glue of the keyframe track as an in-step measurement of hnet_filters (include/hnet.h
// hnet_filters_set_keyframe_measure and hnet_filters_set_keyframe_recover) between the network's last update, the unchanged launches of
// the keyframe track, with or without the recovery of a lost camera inside it, and the filter's own innovation and update kernels: the filter's step as
// the track's step, the track's record as the packed 72-float measurement those kernels take, with the source of the measurement picked per slot, and
// what became of it, with the relocalise records assembled behind the measure records.  ONE measure and ONE finish kernel serve the plain and the
// recovering track: the rule is include/hnet_keyframe_measure_recover.h's, which on a record without RECOVERED is include/hnet_keyframe_measure.h's bit
// for bit.  One wavefront per slot; fp64, serial on lane 0 where the rule is serial, and like kernels_filters_refine.hip built with -ffp-contract=off:
// element (t >> 3, t & 7) of the matrices on lane t, in the collective body shared with the fallback (filters_measure_dev.h), and the inverse is
// invert8_lanes.  No atomics, no scratch memory, nothing waits on another workgroup; ids and slots are bounds-checked here.  The host side that enqueues
// these kernels is capi_filters.hip.
#include "filters_keyframe_dev.h"
#include "filters_measure_dev.h"

namespace hnet {

namespace rf = hnet_refine;
namespace kfm = hnet_kfm;
namespace kfmr = hnet_kfmr;
namespace kr = hnet_keyframe_recovery;

static_assert(offsetof(KfmRec, flags) == (KFM_REC_DOUBLES - 1) * sizeof(double) && sizeof(KeyTrack) % sizeof(double) == 0 && offsetof(KfmRec, track) == 0,
              "KfmRec: the track first, doubles throughout, then flags | pad");
static_assert(offsetof(KfmRec, s_diag) == offsetof(KfmRec, r) + 8 * sizeof(double) && offsetof(KfmRec, nis) == offsetof(KfmRec, r) + 16 * sizeof(double),
              "KfmRec: r, s_diag, nis as in InnovRec");
static_assert(offsetof(RecoverRec, track) == 0 && offsetof(RecoverRec, reloc) == sizeof(KeyTrack) && sizeof(OrientedRelocRec) == (size_t)kr::RELOC_WORDS * 4,
              "RecoverRec: the track, then the relocalise record as 32-bit words");

__global__ __launch_bounds__(KFM_THREADS) void filter_kfm_step_kernel(const int32_t* __restrict__ ids, int n, int n_sessions, const KfmCfg* __restrict__ cfg,
                                                                      const FilterRec* __restrict__ work, float* __restrict__ step, KfmRec* __restrict__ out) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return;
    const int id = ids[b];
    const bool asked = id >= 0 && id < n_sessions && cfg[id].on != 0;            // (uniform over the workgroup)
    double* ow = reinterpret_cast<double*>(out + b);
    for (int i = t; i < KFM_REC_DOUBLES - 1; i += KFM_THREADS) ow[i] = 0.0;
    __syncthreads();                                                            // (step_px lies inside the doubles zeroed above)
    if (t == 0) { out[b].flags = asked ? kfm::ASKED : 0; out[b].pad = 0; }
    if (t < 8) {
        const float v = asked ? kfm::step_entry(work[b].s, t) : __int_as_float(0x7fc00000);
        step[(size_t)b * 8 + t] = v;
        if (asked) out[b].step_px[t] = v;
    }
}

// (track, reloc: slot b's records lie b * stride bytes behind them)
__global__ __launch_bounds__(KFM_THREADS) void filter_kfm_measure_kernel(const int32_t* __restrict__ ids, int n, int n_sessions, const FilterParams* __restrict__ params,
                                                                         const KfmCfg* __restrict__ cfg, const KeyState* __restrict__ key_state,
                                                                         const int32_t* __restrict__ prev_ok, const uint8_t* __restrict__ track,
                                                                         const uint8_t* __restrict__ reloc, int stride, const int32_t* __restrict__ accepted,
                                                                         const RobustRec* __restrict__ rec, int levels, const int32_t* __restrict__ updates,
                                                                         float* __restrict__ m72, int32_t* __restrict__ gate, int32_t* __restrict__ opened, KfmRec* out) {
    __shared__ double M[64], V[64], L[64];
    __shared__ rf::Bright f;
    __shared__ int why, bad;
    __shared__ float z[8];
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return;
    const int id = ids[b];
    if (id < 0 || id >= n_sessions || !(out[b].flags & kfm::ASKED)) {            // (uniform over the workgroup, as every return below)
        if (t == 0) { gate[b] = 0; opened[b] = -1; }
        return;
    }
    const KeyTrack& tr = *reinterpret_cast<const KeyTrack*>(track + (size_t)b * stride);
    const OrientedRelocRec* rl = reloc ? reinterpret_cast<const OrientedRelocRec*>(reloc + (size_t)b * stride) : nullptr;
    const bool from = rl && kfmr::from_reloc(tr.flags);                          // (read only where no reason was found: then RL_RETRACKED)
    const RobustRec& r0 = from ? rl->rv.rec : tr.rec;
    const double kc = params[id].k_net_cov;
    const KfmCfg cf = cfg[id];
    const int upd = updates[b];
    const bool sel = kfm::selected(cf.when, upd);
    const double* src = reinterpret_cast<const double*>(&tr);
    double* dst = reinterpret_cast<double*>(&out[b].track);
    for (int i = t; i < (int)(sizeof(KeyTrack) / sizeof(double)); i += KFM_THREADS) dst[i] = src[i];
    int pre = 0, acc = 0;
    if (t == 0) {
        const KeyState& ks = key_state[id];
        pre = kfmr::usable_recover(ks.has_key != 0, tr.flags, rl ? rl->rv.flags : 0, prev_ok[id]);
        if (!pre && !kfm::relative_z(ks.key_px, r0.px.offsets_px, z)) pre = kfm::NO_INVERSE;
        if (!pre) {
            if (accepted && !from) acc = accepted[b];                            // (the relocalisation's alignment has reused rec: the track's count was kept)
            else
                for (int l = 0; l < levels; l++) acc += rec[(size_t)l * n + b].px.accepted;
        }
    }
    double R;
    const int reason = refine_measure_lanes(r0, acc, pre, cf.max_mse, cf.cov_scale, cf.sigma_floor_px, kc, M, V, L, f, why, bad, R);
    const int skipped = sel ? 0 : (int)kfm::NOT_SELECTED;
    if (reason) {
        if (t == 0) { out[b].flags = kfm::ASKED | reason | skipped; gate[b] = 0; opened[b] = -1; }
        return;
    }
    out[b].r_px[t] = R;
    m72[(size_t)b * 72 + 8 + t] = rf::cov72_entry(R, kc);
    if (t < 8) {
        m72[(size_t)b * 72 + t] = z[t];
        out[b].z_px[t] = z[t];
    }
    if (t == 0) {
        out[b].flags = kfm::ASKED | skipped | (from ? (int)kfmr::FROM_RELOC : 0);
        gate[b] = sel ? 1 : 0;
        opened[b] = sel ? upd : -1;
    }
}

__global__ __launch_bounds__(KFM_THREADS) void filter_kfm_finish_kernel(const int32_t* __restrict__ ids, int n, int n_sessions, const InnovRec* __restrict__ innov,
                                                                        const int32_t* __restrict__ updates, const int32_t* __restrict__ opened, int iters,
                                                                        const RecoverRec* __restrict__ rout, int32_t* __restrict__ prev_ok_next, KfmRec* out,
                                                                        OrientedRelocRec* __restrict__ reloc_out) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return;
    if (reloc_out) {
        const uint32_t* rs = reinterpret_cast<const uint32_t*>(&rout[b].reloc);
        uint32_t* ro = reinterpret_cast<uint32_t*>(reloc_out + b);
        for (int i = t; i < kr::RELOC_WORDS; i += KFM_THREADS) ro[i] = rs[i];
    }
    const int id = ids[b];
    if (id < 0 || id >= n_sessions || !(out[b].flags & kfm::ASKED)) return;
    const int before = opened[b];
    const InnovRec& in = innov[b];
    if (before >= 0 && t < 17) out[b].r[t] = reinterpret_cast<const double*>(&in)[t];        // r | s_diag | nis are 17 doubles in both records
    if (t == 0) {
        out[b].iteration = iters;
        out[b].flag = before >= 0 ? in.flag : (int)hnet_ekf::INNOV_NONE;
        int fl = out[b].flags;
        if (before >= 0) {
            if (in.flag == hnet_ekf::INNOV_REJECTED) fl |= kfm::NIS_REJECTED;
            else if (updates[b] < 0) fl |= kfm::S_SINGULAR;
            else if (updates[b] > before) fl |= kfm::APPLIED;
        }
        out[b].flags = fl;
        prev_ok_next[id] = kfmr::next_prev_ok_recover(out[b].track.flags);
    }
}

hipError_t launch_filter_kfm_step(const int32_t* ids, int n, int n_sessions, const KfmCfg* cfg, const FilterRec* work, float* step, KfmRec* out, hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_kfm_step_kernel, dim3((unsigned)n), dim3(KFM_THREADS), 0, s, ids, n, n_sessions, cfg, work, step, out);
    return hipGetLastError();
}

hipError_t launch_filter_kfm_measure(const int32_t* ids, int n, int n_sessions, const FilterParams* params, const KfmCfg* cfg, const KeyState* key_state,
                                     const int32_t* prev_ok, const KeyTrack* track, const RecoverRec* rout, const int32_t* accepted, const RobustRec* rec, int levels,
                                     const int32_t* updates, float* m72, int32_t* gate, int32_t* opened, KfmRec* out, hipStream_t s) {
    if (n < 1 || levels < 1 || levels > hnet_align::MAX_LEVELS || !track == !rout || (rout && !accepted)) return hipErrorInvalidValue;
    const uint8_t* tr = reinterpret_cast<const uint8_t*>(rout ? &rout->track : track);
    const uint8_t* rl = rout ? reinterpret_cast<const uint8_t*>(&rout->reloc) : nullptr;
    hipLaunchKernelGGL(filter_kfm_measure_kernel, dim3((unsigned)n), dim3(KFM_THREADS), 0, s, ids, n, n_sessions, params, cfg, key_state, prev_ok, tr, rl,
                       (int)(rout ? sizeof(RecoverRec) : sizeof(KeyTrack)), accepted, rec, levels, updates, m72, gate, opened, out);
    return hipGetLastError();
}

hipError_t launch_filter_kfm_finish(const int32_t* ids, int n, int n_sessions, const InnovRec* innov, const int32_t* updates, const int32_t* opened, int iters,
                                    const RecoverRec* rout, int32_t* prev_ok_next, KfmRec* out, OrientedRelocRec* reloc_out, hipStream_t s) {
    if (n < 1 || !rout != !reloc_out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_kfm_finish_kernel, dim3((unsigned)n), dim3(KFM_THREADS), 0, s, ids, n, n_sessions, innov, updates, opened, iters, rout, prev_ok_next, out,
                       reloc_out);
    return hipGetLastError();
}

}  // namespace hnet
