// filters_dev.h — what the device filters (hnet_filters, include/hnet.h) and their host orchestration in capi_sessions.hip share.
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

}  // namespace hnet
#endif  // HNET_FILTERS_DEV_H
