// filters_dev.h — what the device filters (hnet_filters, include/hnet.h) and their host orchestration in capi_filters.hip share.
// The device compiles the host reference include/hnet_ekf.h itself (host + device functions) so that the Jacobians, the mean
// propagation and the quaternion update are the very functions tests/test_filters_cpu.py pins against numpy; the parallel parts
// (covariance products, the 8 x 8 inverse, the gain) are restated in kernels_filters.hip in the host's summation order.
#ifndef HNET_FILTERS_DEV_H
#define HNET_FILTERS_DEV_H

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>

#pragma clang force_cuda_host_device begin
#include "../../include/hnet_ekf.h"
#pragma clang force_cuda_host_device end

namespace hnet {

// one filter's fixed parameters as the kernels read them (hnet_filters_set_params)
struct FilterParams {
    hnet_ekf::Extrinsics ext;
    double q[hnet_ekf::NW];            // noise_q_diag
    double gravity_mag, k_net_cov;
    int32_t imu_avg, pad;
};

// one filter's state: the layout of hnet_filter_state (t, then hnet_ekf::State)
struct FilterRec {
    double t;
    hnet_ekf::State s;
};
constexpr int FILTER_REC_DOUBLES = (int)(sizeof(FilterRec) / sizeof(double));     // 758
static_assert(sizeof(FilterRec) == 758 * sizeof(double), "FilterRec must be 758 packed doubles");

constexpr int FILTER_THREADS = 256;

// the step's kernels (kernels_filters.hip); grids of n workgroups / threads, every index host-validated and bounds-checked again on the device
hipError_t launch_filter_propagate(const int32_t* ids, int n, int n_sessions, const FilterRec* state, const FilterParams* params,
                                   const hnet_ekf::ImuData* rd, const int32_t* rd_off, const double* t_frame, FilterRec* work, hipStream_t s);
hipError_t launch_filter_prior(const FilterRec* work, int n, float* prior_px, double* prior_cam, hipStream_t s);
hipError_t launch_filter_update(const int32_t* ids, int n, int n_sessions, const FilterParams* params, const float* net72, const double* prior_cam,
                                const int32_t* gate, int update_offset, int last, FilterRec* work, int32_t* updates, hipStream_t s);
hipError_t launch_filter_scatter(const FilterRec* work, const int32_t* ids, int n, int n_sessions, FilterRec* state, hipStream_t s);


// ---- the IMU feed (hnet_filters_enable_feed .. hnet_filters_advance).  Per session a ring of `cap` readings, ring[id * cap + (head + j) % cap] the
// j-th oldest of `count`; head / count live in ImuRingMeta on the device (the kernels read them) and are mirrored on the host (it computes them).
struct ImuRingMeta { int32_t head, count; };
// one session's segment of a feed call: readings fed[src0 .. src0 + n) go to ring positions (wpos + k) % cap; the ring's head / count afterwards
struct ImuFeedSeg { int32_t id, src0, n, wpos, head, count; };
// the initialiser's settings per session (hnet_init_params)
struct InitParams { double window_time, imu_thresh, init_height; int32_t wait_for_jerk, pad; };
// what hnet_filters_advance asks for one listed session (one workgroup of the init / select / propagate kernels each)
struct AdvanceJob {
    double t_frame, cam_imu_dt;
    int32_t id;
    int32_t init;                      // 1: the state comes from the initialiser in this call (work[b], when ok[b]); 0: from state[id]
    int32_t reset;                     // 1: State::reset_4pt_offset after the propagation (a session that takes no part in the forwards)
    int32_t pad;
};
// per listed session, written by the kernels: ok (init == 0: 1; init == 1: the initialiser's decision), the readings selected, the initialiser's time0
struct AdvanceResult { double time0; int32_t ok, n_sel; };

hipError_t launch_imu_append(const ImuFeedSeg* seg, int n_seg, int max_seg_len, const hnet_ekf::ImuData* fed, int n_fed, int n_sessions, int cap,
                             hnet_ekf::ImuData* ring, ImuRingMeta* meta, hipStream_t s);
hipError_t launch_filter_init(const AdvanceJob* job, int n, int n_sessions, int cap, const hnet_ekf::ImuData* ring, const ImuRingMeta* meta,
                              const InitParams* ip, const FilterParams* params, FilterRec* work, AdvanceResult* res, hipStream_t s);
// sel: [n][2 * (cap + 2)] readings (the span copied out of the ring, then the selected readings behind it)
hipError_t launch_filter_select(const AdvanceJob* job, int n, int n_sessions, int cap, const hnet_ekf::ImuData* ring, const ImuRingMeta* meta,
                                const FilterRec* state, const FilterRec* work, hnet_ekf::ImuData* sel, AdvanceResult* res, hipStream_t s);
hipError_t launch_filter_propagate_adv(const AdvanceJob* job, int n, int n_sessions, int cap, const FilterRec* state, const FilterParams* params,
                                       const hnet_ekf::ImuData* sel, const AdvanceResult* res, FilterRec* work, hipStream_t s);
hipError_t launch_filter_scatter_ok(const FilterRec* work, const AdvanceJob* job, const AdvanceResult* res, int n, int n_sessions, FilterRec* state, hipStream_t s);

// ---- prediction between frames (hnet_filters_predict): read-only over the states and the rings.
// what the call asks for one listed session: status is HNET_PRED_OK (the kernel predicts, or reports AT_STATE when t_query <= the state's t) or the
// host's refusal (NO_STATE / WAIT_IMU: the record is zero apart from it)
struct PredictJob {
    double t_query, cam_imu_dt;
    int32_t id, status;
};
constexpr int PRED_OK = 0, PRED_NO_STATE = 1, PRED_WAIT_IMU = 2, PRED_AT_STATE = 3;      // include/hnet.h HNET_PRED_*
// the layout of hnet_odometry: hnet_ekf::Odometry, the pixel prior, intervals and status
struct PredictOut {
    hnet_ekf::Odometry o;
    double prior_px[8];
    int32_t intervals, status;
};
constexpr int PREDICT_OUT_DOUBLES = (int)(sizeof(PredictOut) / sizeof(double));     // 33
static_assert(sizeof(PredictOut) == 33 * sizeof(double), "PredictOut must be 32 packed doubles and two ints");
constexpr int PREDICT_THREADS = 64;
// scratch: [n][2 * (cap + 2)] readings of the call's own (the span, then the selection), never the advance's sel
hipError_t launch_filter_predict(const PredictJob* job, int n, int n_sessions, int cap, const hnet_ekf::ImuData* ring, const ImuRingMeta* meta,
                                 const FilterRec* state, const FilterParams* params, hnet_ekf::ImuData* scratch, PredictOut* out, hipStream_t s);

// ---- prediction between frames with the covariance (hnet_filters_predict_cov): the record of the predict plus the covariance
// hnet_ekf::propagate_with_imu gives at the query time and hnet_ekf::odometry_cov_from_state's blocks of it; read-only like the predict.
// the layout of hnet_odometry_cov: hnet_ekf::OdometryCov
struct PredictCovOut { hnet_ekf::OdometryCov c; };
constexpr int PREDICT_COV_DOUBLES = (int)(sizeof(PredictCovOut) / sizeof(double));  // 118
static_assert(sizeof(PredictCovOut) == 118 * sizeof(double), "PredictCovOut must be 118 packed doubles");
// one workgroup of FILTER_THREADS per job.  scratch as launch_filter_predict's (the two calls are ordered on one stream and may share it);
// out [n], cov_out [n]; full: null or [n][729], the propagated covariance itself
hipError_t launch_filter_predict_cov(const PredictJob* job, int n, int n_sessions, int cap, const hnet_ekf::ImuData* ring, const ImuRingMeta* meta,
                                     const FilterRec* state, const FilterParams* params, hnet_ekf::ImuData* scratch, PredictOut* out,
                                     PredictCovOut* cov_out, double* full, hipStream_t s);

// ---- innovation records and the NIS gate (hnet_filters_enable_innovations).
// the layout of hnet_innovation: hnet_ekf::Innovation's r, s_diag and nis, then the iteration and the flag (hnet_ekf::INNOV_*)
struct InnovRec {
    double r[8], s_diag[8], nis;
    int32_t iteration, flag;
};
constexpr int INNOV_REC_DOUBLES = (int)(sizeof(InnovRec) / sizeof(double));       // 18
static_assert(sizeof(InnovRec) == 18 * sizeof(double), "InnovRec must be 17 packed doubles and two ints");
constexpr int INNOV_THREADS = 64;
// iteration `it` of a step of n sessions, between its forward and its filter_update_kernel: writes innov[it * n + b] and, on a rejection, 0 to gate[b]
// (the step's device copy, uploaded again by every attempt).  max_nis: [n_sessions], <= 0 = no gate.  Reads innov[(it - 1) * n + b] for it > 0.
// photo_verdict: null, or the [n] verdict words of photo_gate_kernel (photo_dev.h) in a step with a photometric gate: non-zero -> SKIPPED.
hipError_t launch_filter_innovation(const int32_t* ids, int n, int n_sessions, const FilterParams* params, const FilterRec* work, const float* net72,
                                    const double* prior_cam, const double* max_nis, int32_t* gate, const int32_t* updates, int it, InnovRec* innov,
                                    const int32_t* photo_verdict, hipStream_t s);

}  // namespace hnet
#endif  // HNET_FILTERS_DEV_H
