// kernels_filters.hip — the device side of hnet_filters (include/hnet.h): the per-frame filter work of VioManager.cpp:188-275 for many
// sessions at once, fp64 throughout.  One workgroup of 256 threads per listed session; the session's state (758 doubles, 5.9 KB) lives in
// LDS for the whole launch.  Serial parts (Jacobians, mean, quaternion update) run on one lane with the host reference's own functions
// (filters_dev.h); the products run one output element per thread with the k-loop in the host's order.  The Makefile builds this file
// with -ffp-contract=off (a per-target flag: the pragma form would only cover code after the include of include/hnet_ekf.h), so the header's
// serial code and the products round every multiply and add as the host's x86-64 build does; device and host then differ only where the
// device library's sin / cos / sqrt / division do.
#include "filters_dev.h"

namespace hnet {

namespace {
constexpr int NS = hnet_ekf::NS, NW = hnet_ekf::NW;
constexpr int NE = NS * NS;                                   // 729 covariance elements
constexpr int EPT = (NE + FILTER_THREADS - 1) / FILTER_THREADS;   // 3 per thread

__device__ inline void load_rec(FilterRec& dst, const FilterRec& src) {
    const double* s = reinterpret_cast<const double*>(&src);
    double* d = reinterpret_cast<double*>(&dst);
    for (int i = threadIdx.x; i < FILTER_REC_DOUBLES; i += FILTER_THREADS) d[i] = s[i];
}
__device__ inline void store_rec(FilterRec& dst, const FilterRec& src) {
    const double* s = reinterpret_cast<const double*>(&src);
    double* d = reinterpret_cast<double*>(&dst);
    for (int i = threadIdx.x; i < FILTER_REC_DOUBLES; i += FILTER_THREADS) d[i] = s[i];
}
// row of the state that measurement component j selects (update(): 15 + 3c + k)
__device__ inline int sel(int j) { return 15 + 3 * (j >> 1) + (j & 1); }
}  // namespace

// IMU propagation of session ids[b] over its selected readings rd[rd_off[b] .. rd_off[b + 1]) (hnet_ekf::propagate_with_imu's loop):
// per interval the corrected inputs with the current biases, the Jacobians and the mean on lane 0, then P <- F P F^T + Fw diag(q) Fw^T
// by all lanes.  The result goes to work[b] with time t_frame[b].
__global__ __launch_bounds__(FILTER_THREADS) void filter_propagate_kernel(const int32_t* __restrict__ ids, int n_sessions, const FilterRec* __restrict__ state,
                                                                          const FilterParams* __restrict__ params, const hnet_ekf::ImuData* __restrict__ rd,
                                                                          const int32_t* __restrict__ rd_off, const double* __restrict__ t_frame,
                                                                          FilterRec* __restrict__ work) {
    __shared__ FilterRec S;
    __shared__ double F[NE], Fw[NS * NW], T[NE];
    const int b = blockIdx.x, id = ids[b];
    if (id < 0 || id >= n_sessions) return;                   // (host-validated)
    const FilterParams& pr = params[id];
    load_rec(S, state[id]);
    const int k0 = rd_off[b], k1 = rd_off[b + 1];
    __syncthreads();
    for (int k = k0; k + 1 < k1; k++) {
        if (threadIdx.x == 0) {
            double w_hat[3], a_hat[3];
            const double dt = hnet_ekf::imu_interval_inputs(S.s, rd[k], rd[k + 1], pr.imu_avg != 0, w_hat, a_hat);
            hnet_ekf::propagate_jacobians(S.s, pr.ext, dt, w_hat, F, Fw, pr.gravity_mag);
            hnet_ekf::propagate_mean(S.s, pr.ext, dt, w_hat, a_hat, pr.gravity_mag);
        }
        __syncthreads();
        for (int e = threadIdx.x; e < NE; e += FILTER_THREADS) {              // T = F P
            const int i = e / NS, j = e % NS;
            double a = 0.0;
            for (int q = 0; q < NS; q++) a += F[i * NS + q] * S.s.cov[q * NS + j];
            T[e] = a;
        }
        __syncthreads();
        double o[EPT];
        for (int r = 0; r < EPT; r++) {                                         // T F^T + Fw diag(q) Fw^T
            const int e = threadIdx.x + r * FILTER_THREADS;
            if (e >= NE) break;
            const int i = e / NS, j = e % NS;
            double a = 0.0;
            for (int q = 0; q < NS; q++) a += T[i * NS + q] * F[j * NS + q];
            for (int q = 0; q < NW; q++) a += Fw[i * NW + q] * pr.q[q] * Fw[j * NW + q];
            o[r] = a;
        }
        for (int r = 0; r < EPT; r++) {
            const int e = threadIdx.x + r * FILTER_THREADS;
            if (e < NE) S.s.cov[e] = o[r];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) S.t = t_frame[b];
    __syncthreads();
    store_rec(work[b], S);
}

// VioManager.cpp:230-234 + the (float) cast of hnet_sessions_infer: prior_px[b][k] = (float)(offset * 159.5), prior_cam[b][k] = offset
__global__ __launch_bounds__(256) void filter_prior_kernel(const FilterRec* __restrict__ work, int n, float* __restrict__ prior_px, double* __restrict__ prior_cam) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= 8 * n) return;
    const int b = g >> 3, c = (g & 7) >> 1, k = g & 1;
    const double off = work[b].s.offset[c][k];
    prior_cam[g] = off;
    prior_px[g] = (float)(off * hnet_ekf::F_PIX);
}

// UpdaterHNet::update (hnet_ekf::update) of work[b] with the network's packed record net72[b] (mean 8 | cov 64), when gate[b] and no earlier
// update of this step found S singular (updates[b] >= 0); a singular S leaves the state as it was and sets updates[b] = -1 - updates[b].
// `last`: State::reset_4pt_offset afterwards, gated or not.
__global__ __launch_bounds__(FILTER_THREADS) void filter_update_kernel(const int32_t* __restrict__ ids, int n_sessions, const FilterParams* __restrict__ params,
                                                                       const float* __restrict__ net72, const double* __restrict__ prior_cam,
                                                                       const int32_t* __restrict__ gate, int update_offset, int last,
                                                                       FilterRec* __restrict__ work, int32_t* __restrict__ updates) {
    __shared__ FilterRec S;
    __shared__ double A[64], V[64], PHt[NS * 8], K[NS * 8], dx[NS], inno[8];
    const int b = blockIdx.x, id = ids[b];
    if (id < 0 || id >= n_sessions) return;
    const int done = updates[b];
    const bool run = gate[b] != 0 && done >= 0;
    if (!run && !last) return;                                                 // (uniform over the workgroup)
    load_rec(S, work[b]);
    __syncthreads();
    const int t = threadIdx.x;
    if (run) {
        const double kc = params[id].k_net_cov;
        const float* nm = net72 + (size_t)b * 72;
        if (t < 64) {
            const int i = t >> 3, j = t & 7;
            A[t] = S.s.cov[sel(i) * NS + sel(j)] + kc * (double)nm[8 + t] / (hnet_ekf::F_PIX * hnet_ekf::F_PIX);
            V[t] = i == j ? 1.0 : 0.0;
        }
        for (int e = t; e < NS * 8; e += FILTER_THREADS) PHt[e] = S.s.cov[(e >> 3) * NS + sel(e & 7)];
        if (t < 8) inno[t] = (double)nm[t] / hnet_ekf::F_PIX - prior_cam[(size_t)b * 8 + t];
        __syncthreads();
        // hnet_ekf::invert(A, 8): Gauss-Jordan with partial pivoting, the same operations in the same order, rows / columns across lanes
        bool singular = false;
        for (int col = 0; col < 8; col++) {
            int piv = col;
            for (int r = col + 1; r < 8; r++)
                if (fabs(A[r * 8 + col]) > fabs(A[piv * 8 + col])) piv = r;
            if (A[piv * 8 + col] == 0.0) { singular = true; break; }             // (every lane sees the same LDS values)
            __syncthreads();
            if (piv != col && t < 16) {
                double* X = t < 8 ? A : V;
                const int j = t & 7;
                const double tmp = X[col * 8 + j];
                X[col * 8 + j] = X[piv * 8 + j];
                X[piv * 8 + j] = tmp;
            }
            __syncthreads();
            const double d = 1.0 / A[col * 8 + col];
            __syncthreads();
            if (t < 16) (t < 8 ? A : V)[col * 8 + (t & 7)] *= d;
            __syncthreads();
            const int r = t >> 4, j = t & 7;
            double* X = (t & 8) ? V : A;
            const double f = t < 128 ? A[r * 8 + col] : 0.0;
            __syncthreads();
            if (t < 128 && r != col && f != 0.0) X[r * 8 + j] -= f * X[col * 8 + j];
            __syncthreads();
        }
        if (singular) {
            if (t == 0) updates[b] = -1 - done;
        } else {
            for (int e = t; e < NS * 8; e += FILTER_THREADS) {                  // K = P H^T S^-1
                const int i = e >> 3, j = e & 7;
                double a = 0.0;
                for (int q = 0; q < 8; q++) a += PHt[i * 8 + q] * V[q * 8 + j];
                K[e] = a;
            }
            __syncthreads();
            double o[EPT];
            for (int r = 0; r < EPT; r++) {                                     // (K H) P
                const int e = t + r * FILTER_THREADS;
                if (e >= NE) break;
                const int i = e / NS, j = e % NS;
                double a = 0.0;
                for (int q = 0; q < 8; q++) a += K[i * 8 + q] * S.s.cov[sel(q) * NS + j];
                o[r] = a;
            }
            if (t < NS) {
                double a = 0.0;
                if (update_offset || t < 15)
                    for (int q = 0; q < 8; q++) a += K[t * 8 + q] * inno[q];
                dx[t] = a;
            }
            __syncthreads();
            for (int r = 0; r < EPT; r++) {
                const int e = t + r * FILTER_THREADS;
                if (e < NE) S.s.cov[e] -= o[r];
            }
            if (t == 0) {
                hnet_ekf::State& s = S.s;
                for (int i = 0; i < 3; i++) s.p[i] += dx[i];
                hnet_ekf::quat_apply_rotvec(dx + 3, s.q);
                for (int i = 0; i < 3; i++) { s.v[i] += dx[6 + i]; s.ba[i] += dx[9 + i]; s.bg[i] += dx[12 + i]; }
                if (update_offset)
                    for (int c = 0; c < 4; c++)
                        for (int k = 0; k < 3; k++) s.offset[c][k] += dx[15 + 3 * c + k];
                updates[b] = done + 1;
            }
        }
        __syncthreads();
    }
    if (last) {                                                                // hnet_ekf::reset_4pt_offset
        for (int e = t; e < NE; e += FILTER_THREADS)
            if (e / NS >= 15 || e % NS >= 15) S.s.cov[e] = 0.0;
        if (t < 12) (&S.s.offset[0][0])[t] = 0.0;
        __syncthreads();
    }
    store_rec(work[b], S);
}

// the step's result work[b] -> state[ids[b]] (after the host accepted the step's forwards)
__global__ __launch_bounds__(FILTER_THREADS) void filter_scatter_kernel(const FilterRec* __restrict__ work, const int32_t* __restrict__ ids, int n_sessions,
                                                                        FilterRec* __restrict__ state) {
    const int b = blockIdx.x, id = ids[b];
    if (id < 0 || id >= n_sessions) return;
    store_rec(state[id], work[b]);
}

hipError_t launch_filter_propagate(const int32_t* ids, int n, int n_sessions, const FilterRec* state, const FilterParams* params, const hnet_ekf::ImuData* rd,
                                   const int32_t* rd_off, const double* t_frame, FilterRec* work, hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_propagate_kernel, dim3((unsigned)n), dim3(FILTER_THREADS), 0, s, ids, n_sessions, state, params, rd, rd_off, t_frame, work);
    return hipGetLastError();
}

hipError_t launch_filter_prior(const FilterRec* work, int n, float* prior_px, double* prior_cam, hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_prior_kernel, dim3((unsigned)((8 * n + 255) / 256)), dim3(256), 0, s, work, n, prior_px, prior_cam);
    return hipGetLastError();
}

hipError_t launch_filter_update(const int32_t* ids, int n, int n_sessions, const FilterParams* params, const float* net72, const double* prior_cam,
                                const int32_t* gate, int update_offset, int last, FilterRec* work, int32_t* updates, hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_update_kernel, dim3((unsigned)n), dim3(FILTER_THREADS), 0, s, ids, n_sessions, params, net72, prior_cam, gate, update_offset,
                       last, work, updates);
    return hipGetLastError();
}

hipError_t launch_filter_scatter(const FilterRec* work, const int32_t* ids, int n, int n_sessions, FilterRec* state, hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_scatter_kernel, dim3((unsigned)n), dim3(FILTER_THREADS), 0, s, work, ids, n_sessions, state);
    return hipGetLastError();
}

}  // namespace hnet
