// filters_refine_dev.h — the photometric fallback of hnet_filters (include/hnet.h hnet_filters_set_photo_refine): what capi_filters.hip and
// kernels_filters_refine.hip share.  The device compiles include/hnet_photo_refine.h itself (host + device functions): the marginal, the pivot test and
// the entries of R_px are the functions tests/test_filters_photo_refine_cpu.py pins on the host.
#pragma once
#include "filters_dev.h"
#include "photo_robust_dev.h"

#pragma clang force_cuda_host_device begin
#include "../../include/hnet_photo_refine.h"
#pragma clang force_cuda_host_device end

namespace hnet {

using RefineRec = hnet_refine::Record;       // = hnet_photo_refine
using RefineOpts = hnet_refine::Opts;        // = hnet_photo_refine_opts
static_assert(sizeof(RefineRec) == sizeof(RobustRec) + 64 * sizeof(double) + sizeof(InnovRec) + 8 && offsetof(RefineRec, r) == sizeof(RobustRec) + 64 * sizeof(double) &&
              offsetof(RefineRec, flags) == offsetof(RefineRec, r) + sizeof(InnovRec) && sizeof(RefineOpts) == sizeof(RobustOpts) + 32, "packed layouts");
constexpr int REFINE_REC_DOUBLES = (int)(sizeof(RefineRec) / sizeof(double));     // 278
constexpr int REFINE_THREADS = 64;

// one session's refinement as the kernels read it: on = 0 is off (hnet_filters_set_photo_refine)
struct RefineCfg { double cov_scale, sigma_floor_px, max_mse; int32_t on, pad; };

// One wavefront per slot b < n, before the alignment.  Selected iff verdict[b] == 1 (photo_gate_kernel refused iteration 0), cfg[ids[b]].on and
// updates[b] == 0: out[b] = {flags ASKED, zeros} and x0[b] = prior0[b] (iteration 0's fp32 prior); otherwise out[b] = zeros and x0[b] = quiet NaNs, on
// which every level of the alignment reports DEGENERATE and its later workgroups return at once.
hipError_t launch_filter_refine_select(const int32_t* ids, int n, int n_sessions, const RefineCfg* cfg, const int32_t* verdict, const int32_t* updates,
                                       const float* prior0, float* x0, RefineRec* out, hipStream_t s);
// One wavefront per slot, after the alignment (rec: [levels][n]).  Selected slots: the level-0 record goes into out[b], hnet_refine's measurement with
// the session's k_net_cov into m72[b] (72 floats) and out[b].r_px, and gate[b] = 1; an unusable record sets its reason bit and gate[b] = 0.
// Unselected slots: gate[b] = 0.  gate is the step's device copy, which nothing reads after the last iteration's update but the fallback's launches.
hipError_t launch_filter_refine_measure(const int32_t* ids, int n, int n_sessions, const FilterParams* params, const RefineCfg* cfg, const RobustRec* rec, int levels,
                                        float* m72, int32_t* gate, RefineRec* out, hipStream_t s);
// After the fallback's innovation and update launches: the innovation record (iteration = iters) and APPLIED / NIS_REJECTED / S_SINGULAR of selected slots
hipError_t launch_filter_refine_finish(int n, const InnovRec* innov, const int32_t* updates, int iters, RefineRec* out, hipStream_t s);
// (State::reset_4pt_offset of every slot, with or without a measurement, is the fallback's filter_update_kernel launch with last = 1)

}  // namespace hnet
