// filters_measure_dev.h - the one workgroup-collective body of the filter's photometric measurements: kernels_filters_refine.hip's fallback
// and kernels_filters_keyframe.hip's keyframe measurement both call it.  Device only.
#pragma once
#include "filters_refine_dev.h"
#include "filters_invert_dev.h"

namespace hnet {
namespace {
// hnet_refine::refine_measurement's matrix part on the record r0, element (t >> 3, t & 7) on lane t of a 64-thread workgroup: precheck, marginal_factor,
// marginal_info, has_factor, the inverse, r_px_entry, in the header's order with the header's operations.  Lane 0's `pre` is a reason found before the
// call (0: none) and its `accepted` the trials accepted over the alignment's levels; no other lane's are read.  The kernel's LDS: the marginal
// information M [64], its inverse V [64] (M and V of invert8_lanes), the factor L [64] of the pivot test, the brightness block f of the marginal and
// the two words `why` and `bad` that lane 0 and the lanes publish.  Every thread of the workgroup calls it (six barriers besides invert8_lanes's own).
// -> the reason bit, 0: lane t's R is element t of R_px and V holds the inverse.
__device__ inline int refine_measure_lanes(const RobustRec& r0, int accepted, int pre, double max_mse, double cov_scale, double sigma_floor_px, double k_net_cov,
                                           double* M, double* V, double* L, hnet_refine::Bright& f, int& why, int& bad, double& R) {
    namespace rf = hnet_refine;
    const int t = threadIdx.x;
    if (t == 0) {
        int w = pre;
        if (!w) w = rf::precheck(r0, accepted, max_mse, k_net_cov);
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
    const bool singular = !why && invert8_lanes(M, V);                     // (V = inverse(info8); every lane read `why` behind the barrier above)
    __syncthreads();
    if (singular && t == 0) why = rf::NO_FACTOR;
    __syncthreads();
    R = 0.0;
    if (!why) {
        R = rf::r_px_entry(V, r0.px.mse, cov_scale, sigma_floor_px, i, j);
        if (!std::isfinite(R)) bad = 1;
    }
    __syncthreads();
    return why ? why : bad ? (int)rf::NON_FINITE : 0;
}
}  // namespace
}  // namespace hnet
