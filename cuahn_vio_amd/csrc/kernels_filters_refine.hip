// kernels_filters_refine.hip — the device glue of the photometric fallback of hnet_filters (include/hnet.h hnet_filters_set_photo_refine)
// between photo_gate_kernel's verdicts, launch_photo_align_robust and the filter's own innovation and update kernels: which slots of a step align, the
// alignment's record as the packed 72-float measurement those kernels take, and what became of it.  One wavefront per slot; fp64 and, like
// kernels_filters.hip, built with -ffp-contract=off: the measurement is include/hnet_photo_refine.h's, element (t >> 3, t & 7) on lane t, in the
// collective body it shares with the keyframe measurement (filters_measure_dev.h), and the inverse is invert8_lanes.  No atomics, nothing waits on
// another workgroup.  The host side that enqueues these kernels is capi_filters.hip.
#include "filters_measure_dev.h"

namespace hnet {

namespace rf = hnet_refine;

static_assert(offsetof(RefineRec, flags) == (REFINE_REC_DOUBLES - 1) * sizeof(double) && sizeof(RobustRec) % sizeof(double) == 0, "RefineRec: doubles, then flags | pad");

__global__ __launch_bounds__(REFINE_THREADS) void filter_refine_select_kernel(const int32_t* __restrict__ ids, int n, int n_sessions, const RefineCfg* __restrict__ cfg,
                                                                              const int32_t* __restrict__ verdict, const int32_t* __restrict__ updates,
                                                                              const float* __restrict__ prior0, float* __restrict__ x0, RefineRec* __restrict__ out) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return;
    const int id = ids[b];
    const bool sel = id >= 0 && id < n_sessions && verdict[b] == 1 && cfg[id].on != 0 && updates[b] == 0;        // (uniform over the workgroup)
    double* ow = reinterpret_cast<double*>(out + b);
    for (int i = t; i < REFINE_REC_DOUBLES - 1; i += REFINE_THREADS) ow[i] = 0.0;
    if (t == 0) { out[b].flags = sel ? rf::ASKED : 0; out[b].pad = 0; }
    if (t < 8) x0[(size_t)b * 8 + t] = sel ? prior0[(size_t)b * 8 + t] : __int_as_float(0x7fc00000);
}

__global__ __launch_bounds__(REFINE_THREADS) void filter_refine_measure_kernel(const int32_t* __restrict__ ids, int n, int n_sessions, const FilterParams* __restrict__ params,
                                                                               const RefineCfg* __restrict__ cfg, const RobustRec* __restrict__ rec, int levels,
                                                                               float* __restrict__ m72, int32_t* __restrict__ gate, RefineRec* out) {
    __shared__ double M[64], V[64], L[64];
    __shared__ rf::Bright f;
    __shared__ int why, bad;
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return;
    const int id = ids[b];
    if (id < 0 || id >= n_sessions || !(out[b].flags & rf::ASKED)) {             // (uniform over the workgroup, as every return below)
        if (t == 0) gate[b] = 0;
        return;
    }
    const RobustRec& r0 = rec[b];
    const double kc = params[id].k_net_cov;
    const RefineCfg cf = cfg[id];
    const double* src = reinterpret_cast<const double*>(&r0);
    double* dst = reinterpret_cast<double*>(&out[b].rec);
    for (int i = t; i < (int)(sizeof(RobustRec) / sizeof(double)); i += REFINE_THREADS) dst[i] = src[i];
    int accepted = 0;
    if (t == 0)
        for (int l = 0; l < levels; l++) accepted += rec[(size_t)l * n + b].px.accepted;
    double R;
    const int reason = refine_measure_lanes(r0, accepted, 0, cf.max_mse, cf.cov_scale, cf.sigma_floor_px, kc, M, V, L, f, why, bad, R);
    if (reason) {
        if (t == 0) { out[b].flags = rf::ASKED | reason; gate[b] = 0; }
        return;
    }
    out[b].r_px[t] = R;
    m72[(size_t)b * 72 + 8 + t] = rf::cov72_entry(R, kc);
    if (t < 8) m72[(size_t)b * 72 + t] = r0.px.offsets_px[t];
    if (t == 0) gate[b] = 1;
}

__global__ __launch_bounds__(REFINE_THREADS) void filter_refine_finish_kernel(int n, const InnovRec* __restrict__ innov, const int32_t* __restrict__ updates, int iters,
                                                                              RefineRec* out) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= n || !(out[b].flags & rf::ASKED)) return;
    const InnovRec& in = innov[b];
    if (t < 17) out[b].r[t] = reinterpret_cast<const double*>(&in)[t];           // r | s_diag | nis are 17 doubles in both records
    if (t == 0) {
        out[b].iteration = iters;
        out[b].flag = in.flag;
        int fl = out[b].flags;
        if (in.flag == hnet_ekf::INNOV_REJECTED) fl |= rf::NIS_REJECTED;
        else if (updates[b] < 0) fl |= rf::S_SINGULAR;
        else if (updates[b] > 0) fl |= rf::APPLIED;
        out[b].flags = fl;
    }
}

static_assert(offsetof(RefineRec, s_diag) == offsetof(RefineRec, r) + 8 * sizeof(double) && offsetof(RefineRec, nis) == offsetof(RefineRec, r) + 16 * sizeof(double),
              "RefineRec: r, s_diag, nis as in InnovRec");

hipError_t launch_filter_refine_select(const int32_t* ids, int n, int n_sessions, const RefineCfg* cfg, const int32_t* verdict, const int32_t* updates,
                                       const float* prior0, float* x0, RefineRec* out, hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_refine_select_kernel, dim3((unsigned)n), dim3(REFINE_THREADS), 0, s, ids, n, n_sessions, cfg, verdict, updates, prior0, x0, out);
    return hipGetLastError();
}

hipError_t launch_filter_refine_measure(const int32_t* ids, int n, int n_sessions, const FilterParams* params, const RefineCfg* cfg, const RobustRec* rec, int levels,
                                        float* m72, int32_t* gate, RefineRec* out, hipStream_t s) {
    if (n < 1 || levels < 1 || levels > hnet_align::MAX_LEVELS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_refine_measure_kernel, dim3((unsigned)n), dim3(REFINE_THREADS), 0, s, ids, n, n_sessions, params, cfg, rec, levels, m72, gate, out);
    return hipGetLastError();
}

hipError_t launch_filter_refine_finish(int n, const InnovRec* innov, const int32_t* updates, int iters, RefineRec* out, hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_refine_finish_kernel, dim3((unsigned)n), dim3(REFINE_THREADS), 0, s, n, innov, updates, iters, out);
    return hipGetLastError();
}

}  // namespace hnet
