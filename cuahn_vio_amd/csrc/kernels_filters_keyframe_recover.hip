// kernels_filters_keyframe_recover.hip — the device glue of recovering a lost camera inside the in-step keyframe track of hnet_filters (include/hnet.h
// hnet_filters_set_keyframe_recover): the track's decision in its deferred form for the sessions that recover and in its plain form for those
// that do not, chosen per slot; 7v's measure kernel on the records of a track with recovery, with the source of the measurement picked per slot; and
// 7v's finish with the new prev_ok and the relocalise records assembled behind the measure records.  Everything between them - 7u's finish and note,
// the search, winner, pick, gather and attach kernels, the alignment's sequence, the filter's innovation and update - is the unchanged launch.  One
// wavefront per slot; fp64, serial on lane 0 where the rule is serial, and like kernels_filters_keyframe.hip built with -ffp-contract=off: the rule is
// include/hnet_keyframe_measure_recover.h's, element (t >> 3, t & 7) of the matrices on lane t, and the inverse is invert8_lanes.  No atomics, no scratch
// memory, nothing waits on another workgroup; ids and slots are bounds-checked here.  The host side is capi_filters.hip and capi_keyframe.hip.
#include "filters_keyframe_recover_dev.h"
#include "filters_invert_dev.h"

namespace hnet {

namespace rf = hnet_refine;
namespace kf = hnet_keyframe;
namespace kfm = hnet_kfm;
namespace kfmr = hnet_kfmr;
namespace kr = hnet_keyframe_recovery;

namespace {
constexpr int REC_DOUBLES = (int)(sizeof(RobustRec) / sizeof(double));
constexpr int TRACK_DOUBLES = (int)(sizeof(KeyTrack) / sizeof(double));
static_assert(sizeof(RobustRec) % sizeof(double) == 0 && offsetof(KeyTrack, rec) == 0 && sizeof(KeyTrack) % sizeof(double) == 0, "KeyTrack: the record first, as doubles");
static_assert(offsetof(RecoverRec, track) == 0 && offsetof(RecoverRec, reloc) == sizeof(KeyTrack) && sizeof(OrientedRelocRec) == (size_t)kr::RELOC_WORDS * 4,
              "RecoverRec: the track, then the relocalise record as 32-bit words");
static_assert(offsetof(KfmRec, flags) == (KFM_REC_DOUBLES - 1) * sizeof(double) && offsetof(KfmRec, track) == 0, "KfmRec: the track first, doubles throughout, then flags | pad");
}  // namespace

// recover_decide_kernel or keyframe_decide_kernel, chosen by recover_on
__global__ __launch_bounds__(KFM_THREADS) void filter_kfmr_decide_kernel(KeyTable tab, int n, int n_sessions, const RobustRec* __restrict__ rec, int levels, const float* x0,
                                                                         KeyOpts opts, const int32_t* __restrict__ recover_on, KeyState* state, KeyTrack* out,
                                                                         int32_t* __restrict__ copy, RecoverStash* __restrict__ stash, int32_t* __restrict__ active,
                                                                         int32_t* __restrict__ accepted) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return;
    const int id = tab.ids[b];
    const bool valid = id >= 0 && id < n_sessions;                               // (uniform over the workgroup)
    const bool read = valid && state[id].has_key != 0;                           // (read by every lane before lane 0 writes the state: one wavefront, in order)
    const double* src = reinterpret_cast<const double*>(rec + b);
    double* dst = reinterpret_cast<double*>(out + b);
    for (int i = t; i < REC_DOUBLES; i += KFM_THREADS) dst[i] = read ? src[i] : 0.0;
    if (t != 0) return;
    int acc = 0;
    for (int l = 0; l < levels; l++) acc += rec[(size_t)l * n + b].px.accepted;
    accepted[b] = acc;
    if (!valid) {
        for (int i = REC_DOUBLES; i < TRACK_DOUBLES; i++) dst[i] = 0.0;
        kr::stash_zero(stash[b]);
        copy[b] = 0;
        active[b] = 0;
        return;
    }
    int act = 0;
    if (recover_on[id] != 0) {
        copy[b] = kr::decide_deferred(state[id], x0 + (size_t)b * 8, rec[b], opts, tab.gap[b] != 0, state[id], out[b], stash[b], act);
    } else {
        copy[b] = kf::decide(state[id], x0 + (size_t)b * 8, rec[b], opts, tab.gap[b] != 0, state[id], out[b]);
        kr::stash_zero(stash[b]);
    }
    active[b] = act;
}

__global__ __launch_bounds__(KFM_THREADS) void filter_kfmr_measure_kernel(const int32_t* __restrict__ ids, int n, int n_sessions, const FilterParams* __restrict__ params,
                                                                          const KfmCfg* __restrict__ cfg, const KeyState* __restrict__ key_state,
                                                                          const int32_t* __restrict__ prev_ok, const RecoverRec* __restrict__ rout,
                                                                          const int32_t* __restrict__ accepted, const RobustRec* __restrict__ rec2, int levels2,
                                                                          const int32_t* __restrict__ updates, float* __restrict__ m72, int32_t* __restrict__ gate,
                                                                          int32_t* __restrict__ opened, KfmRec* out) {
    __shared__ double M[64], V[64], L[64];
    __shared__ rf::Bright f;
    __shared__ float z[8];
    __shared__ int why, bad;
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return;
    const int id = ids[b];
    if (id < 0 || id >= n_sessions || !(out[b].flags & kfm::ASKED)) {            // (uniform over the workgroup, as every return below)
        if (t == 0) { gate[b] = 0; opened[b] = -1; }
        return;
    }
    const KeyTrack& tr = rout[b].track;
    const bool from = kfmr::from_reloc(tr.flags);                                // (read only where no reason was found: then RL_RETRACKED)
    const RobustRec& r0 = from ? rout[b].reloc.rv.rec : tr.rec;
    const double kc = params[id].k_net_cov;
    const KfmCfg cf = cfg[id];
    const int upd = updates[b];
    const bool sel = kfm::selected(cf.when, upd);
    const double* src = reinterpret_cast<const double*>(&tr);
    double* dst = reinterpret_cast<double*>(&out[b].track);
    for (int i = t; i < TRACK_DOUBLES; i += KFM_THREADS) dst[i] = src[i];
    if (t == 0) {
        const KeyState& ks = key_state[id];
        int w = kfmr::usable_recover(ks.has_key != 0, tr.flags, rout[b].reloc.rv.flags, prev_ok[id]);
        if (!w && !kfm::relative_z(ks.key_px, r0.px.offsets_px, z)) w = kfm::NO_INVERSE;
        if (!w) {
            int acc = accepted[b];
            if (from) {
                acc = 0;
                for (int l = 0; l < levels2; l++) acc += rec2[(size_t)l * n + b].px.accepted;
            }
            w = rf::precheck(r0, acc, cf.max_mse, kc);
        }
        if (!w && !rf::marginal_factor(r0, f)) w = rf::NO_FACTOR;
        why = w;
        bad = 0;
    }
    __syncthreads();
    const int i = t >> 3, j = t & 7;
    if (!why) {
        M[t] = rf::marginal_info(r0, f, i, j);
        V[t] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    if (!why && t == 0 && !rf::has_factor(M, L)) why = rf::NO_FACTOR;
    __syncthreads();
    const bool singular = !why && invert8_lanes(M, V);                           // (V = inverse(info8); every lane read `why` behind the barrier above)
    __syncthreads();
    if (singular && t == 0) why = rf::NO_FACTOR;
    __syncthreads();
    double R = 0.0;
    if (!why) {
        R = rf::r_px_entry(V, r0.px.mse, cf.cov_scale, cf.sigma_floor_px, i, j);
        if (!std::isfinite(R)) bad = 1;
    }
    __syncthreads();
    const int reason = why ? why : bad ? (int)rf::NON_FINITE : 0;
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

__global__ __launch_bounds__(KFM_THREADS) void filter_kfmr_finish_kernel(const int32_t* __restrict__ ids, int n, int n_sessions, const InnovRec* __restrict__ innov,
                                                                         const int32_t* __restrict__ updates, const int32_t* __restrict__ opened, int iters,
                                                                         const RecoverRec* __restrict__ rout, int32_t* __restrict__ prev_ok_next, KfmRec* out,
                                                                         OrientedRelocRec* __restrict__ reloc_out) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return;
    const uint32_t* rs = reinterpret_cast<const uint32_t*>(&rout[b].reloc);
    uint32_t* ro = reinterpret_cast<uint32_t*>(reloc_out + b);
    for (int i = t; i < kr::RELOC_WORDS; i += KFM_THREADS) ro[i] = rs[i];
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

hipError_t launch_filter_kfmr_decide(const KeyTable& tab, int n, int n_sessions, const RobustRec* rec, int levels, const float* x0, const KeyOpts& opts,
                                     const int32_t* recover_on, KeyState* state, KeyTrack* out, int32_t* copy, RecoverStash* stash, int32_t* active,
                                     int32_t* accepted, hipStream_t s) {
    if (n < 1 || levels < 1 || levels > hnet_align::MAX_LEVELS || !recover_on || !stash || !active || !accepted) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_kfmr_decide_kernel, dim3((unsigned)n), dim3(KFM_THREADS), 0, s, tab, n, n_sessions, rec, levels, x0, opts, recover_on, state, out, copy,
                       stash, active, accepted);
    return hipGetLastError();
}

hipError_t launch_filter_kfmr_measure(const int32_t* ids, int n, int n_sessions, const FilterParams* params, const KfmCfg* cfg, const KeyState* key_state,
                                      const int32_t* prev_ok, const RecoverRec* rout, const int32_t* accepted, const RobustRec* rec2, int levels2, const int32_t* updates,
                                      float* m72, int32_t* gate, int32_t* opened, KfmRec* out, hipStream_t s) {
    if (n < 1 || levels2 < 1 || levels2 > hnet_align::MAX_LEVELS || !rout || !accepted) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_kfmr_measure_kernel, dim3((unsigned)n), dim3(KFM_THREADS), 0, s, ids, n, n_sessions, params, cfg, key_state, prev_ok, rout, accepted, rec2,
                       levels2, updates, m72, gate, opened, out);
    return hipGetLastError();
}

hipError_t launch_filter_kfmr_finish(const int32_t* ids, int n, int n_sessions, const InnovRec* innov, const int32_t* updates, const int32_t* opened, int iters,
                                     const RecoverRec* rout, int32_t* prev_ok_next, KfmRec* out, OrientedRelocRec* reloc_out, hipStream_t s) {
    if (n < 1 || !rout || !reloc_out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_kfmr_finish_kernel, dim3((unsigned)n), dim3(KFM_THREADS), 0, s, ids, n, n_sessions, innov, updates, opened, iters, rout, prev_ok_next, out,
                       reloc_out);
    return hipGetLastError();
}

}  // namespace hnet
