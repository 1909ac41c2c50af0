// kernels_filters_keyframe.hip — the device glue of the keyframe track as an in-step measurement of hnet_filters (include/hnet.h
// hnet_filters_set_keyframe_measure) between the network's last update, the unchanged launches of the keyframe track and the filter's own
// innovation and update kernels: the filter's step as the track's step, the track's record as the packed 72-float measurement those kernels take, and
// what became of it.  One wavefront per slot; fp64, serial on lane 0 where the rule is serial, and like kernels_filters_refine.hip built with
// -ffp-contract=off: the measurement is include/hnet_keyframe_measure.h's, element (t >> 3, t & 7) of the matrices on lane t, and the inverse is
// invert8_lanes.  No atomics, no scratch memory, nothing waits on another workgroup; ids and slots are bounds-checked here.  The host side that enqueues
// these kernels is capi_filters.hip.
#include "filters_keyframe_dev.h"
#include "filters_invert_dev.h"

namespace hnet {

namespace rf = hnet_refine;
namespace kfm = hnet_kfm;

static_assert(offsetof(KfmRec, flags) == (KFM_REC_DOUBLES - 1) * sizeof(double) && sizeof(KeyTrack) % sizeof(double) == 0 && offsetof(KfmRec, track) == 0,
              "KfmRec: the track first, doubles throughout, then flags | pad");
static_assert(offsetof(KfmRec, s_diag) == offsetof(KfmRec, r) + 8 * sizeof(double) && offsetof(KfmRec, nis) == offsetof(KfmRec, r) + 16 * sizeof(double),
              "KfmRec: r, s_diag, nis as in InnovRec");

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

__global__ __launch_bounds__(KFM_THREADS) void filter_kfm_measure_kernel(const int32_t* __restrict__ ids, int n, int n_sessions, const FilterParams* __restrict__ params,
                                                                         const KfmCfg* __restrict__ cfg, const KeyState* __restrict__ key_state,
                                                                         const int32_t* __restrict__ prev_ok, const KeyTrack* __restrict__ track,
                                                                         const RobustRec* __restrict__ rec, int levels, const int32_t* __restrict__ updates,
                                                                         float* __restrict__ m72, int32_t* __restrict__ gate, int32_t* __restrict__ opened, KfmRec* out) {
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
    const KeyTrack& tr = track[b];
    const RobustRec& r0 = tr.rec;
    const double kc = params[id].k_net_cov;
    const KfmCfg cf = cfg[id];
    const int upd = updates[b];
    const bool sel = kfm::selected(cf.when, upd);
    const double* src = reinterpret_cast<const double*>(&tr);
    double* dst = reinterpret_cast<double*>(&out[b].track);
    for (int i = t; i < (int)(sizeof(KeyTrack) / sizeof(double)); i += KFM_THREADS) dst[i] = src[i];
    if (t == 0) {
        const KeyState& ks = key_state[id];
        int w = kfm::usable(ks.has_key != 0, tr.flags, prev_ok[id]);
        if (!w && !kfm::relative_z(ks.key_px, r0.px.offsets_px, z)) w = kfm::NO_INVERSE;
        if (!w) {
            int accepted = 0;
            for (int l = 0; l < levels; l++) accepted += rec[(size_t)l * n + b].px.accepted;
            w = rf::precheck(r0, accepted, cf.max_mse, kc);
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
        out[b].flags = kfm::ASKED | skipped;
        gate[b] = sel ? 1 : 0;
        opened[b] = sel ? upd : -1;
    }
}

__global__ __launch_bounds__(KFM_THREADS) void filter_kfm_finish_kernel(const int32_t* __restrict__ ids, int n, int n_sessions, const InnovRec* __restrict__ innov,
                                                                        const int32_t* __restrict__ updates, const int32_t* __restrict__ opened, int iters,
                                                                        int32_t* __restrict__ prev_ok_next, KfmRec* out) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return;
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
        prev_ok_next[id] = kfm::next_prev_ok(out[b].track.flags);
    }
}

hipError_t launch_filter_kfm_step(const int32_t* ids, int n, int n_sessions, const KfmCfg* cfg, const FilterRec* work, float* step, KfmRec* out, hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_kfm_step_kernel, dim3((unsigned)n), dim3(KFM_THREADS), 0, s, ids, n, n_sessions, cfg, work, step, out);
    return hipGetLastError();
}

hipError_t launch_filter_kfm_measure(const int32_t* ids, int n, int n_sessions, const FilterParams* params, const KfmCfg* cfg, const KeyState* key_state,
                                     const int32_t* prev_ok, const KeyTrack* track, const RobustRec* rec, int levels, const int32_t* updates, float* m72,
                                     int32_t* gate, int32_t* opened, KfmRec* out, hipStream_t s) {
    if (n < 1 || levels < 1 || levels > hnet_align::MAX_LEVELS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_kfm_measure_kernel, dim3((unsigned)n), dim3(KFM_THREADS), 0, s, ids, n, n_sessions, params, cfg, key_state, prev_ok, track, rec, levels,
                       updates, m72, gate, opened, out);
    return hipGetLastError();
}

hipError_t launch_filter_kfm_finish(const int32_t* ids, int n, int n_sessions, const InnovRec* innov, const int32_t* updates, const int32_t* opened, int iters,
                                    int32_t* prev_ok_next, KfmRec* out, hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_kfm_finish_kernel, dim3((unsigned)n), dim3(KFM_THREADS), 0, s, ids, n, n_sessions, innov, updates, opened, iters, prev_ok_next, out);
    return hipGetLastError();
}

}  // namespace hnet
