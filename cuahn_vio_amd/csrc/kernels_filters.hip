// kernels_filters.hip — the device side of hnet_filters (include/hnet.h): the per-frame filter work of VioManager.cpp:188-275 for many
// sessions at once, fp64 throughout.  One workgroup of 256 threads per listed session; the session's state (758 doubles, 5.9 KB) lives in
// LDS for the whole launch.  Serial parts (Jacobians, mean, quaternion update) run on one lane with the host reference's own functions
// (filters_dev.h); the products run one output element per thread with the k-loop in the host's order.  The Makefile builds this file
// with -ffp-contract=off (a per-target flag: the pragma form would only cover code after the include of include/hnet_ekf.h), so the header's
// serial code and the products round every multiply and add as the host's x86-64 build does; device and host then differ only where the
// device library's sin / cos / sqrt / division do.  The host side that enqueues these kernels is capi_filters.hip.
#include "filters_dev.h"
#include "filters_invert_dev.h"

namespace hnet {

namespace {
constexpr int NS = hnet_ekf::NS, NW = hnet_ekf::NW;
constexpr int NE = NS * NS;                                   // 729 covariance elements
constexpr int EPT = (NE + FILTER_THREADS - 1) / FILTER_THREADS;   // 3 per thread

// one record to another (global memory or LDS on either side) by the FILTER_THREADS lanes of a workgroup
__device__ inline void copy_rec(FilterRec& dst, const FilterRec& src) {
    const double* s = reinterpret_cast<const double*>(&src);
    double* d = reinterpret_cast<double*>(&dst);
    for (int i = threadIdx.x; i < FILTER_REC_DOUBLES; i += FILTER_THREADS) d[i] = s[i];
}
// row of the state that measurement component j selects (update(): 15 + 3c + k)
__device__ inline int sel(int j) { return 15 + 3 * (j >> 1) + (j & 1); }

// hnet_ekf::reset_4pt_offset on the LDS-resident state by the FILTER_THREADS lanes (no barrier of its own: the caller's next one publishes it)
__device__ inline void reset_offset_block(FilterRec& S) {
    for (int e = threadIdx.x; e < NE; e += FILTER_THREADS)
        if (e / NS >= 15 || e % NS >= 15) S.s.cov[e] = 0.0;
    if (threadIdx.x < 12) (&S.s.offset[0][0])[threadIdx.x] = 0.0;
}

// F and Fw as cov_interval wants them before a launch's first interval: zeroed once by all lanes, published by the caller's next barrier
__device__ inline void clear_jacobians(double* F, double* Fw) {
    for (int i = threadIdx.x; i < NE; i += FILTER_THREADS) F[i] = 0.0;
    for (int i = threadIdx.x; i < NS * NW; i += FILTER_THREADS) Fw[i] = 0.0;
}
// One IMU interval [r0, r1] of hnet_ekf::propagate_with_imu's loop on the LDS-resident state S with the LDS arrays F [729], Fw [27 * 15] and T [729], for a
// workgroup of FILTER_THREADS: lane 0 forms the corrected inputs with the current biases, the Jacobians and the mean; all lanes then T = F P and
// P <- T F^T + Fw diag(q) Fw^T, one output element per lane per pass with the k-loop in the host's order.  The Jacobians come from the header's
// propagate_jacobians_fill, which writes the same entries in every interval and touches no other: clear_jacobians once per launch gives what
// propagate_jacobians' per-interval clearing gives (include/hnet_ekf.h).  Contains barriers: every call is uniform over the workgroup; S is
// published on entry (a barrier behind whatever wrote it) and on return.  filter_propagate_kernel calls it; filter_predict_cov_kernel restates the
// body, because as this function it costs that kernel 3 %, and tests/test_gpu_filters_predict_cov.py pins the two bit for bit.
__device__ __forceinline__ void cov_interval(FilterRec& S, const FilterParams& pr, const hnet_ekf::ImuData& r0, const hnet_ekf::ImuData& r1, double* F, double* Fw, double* T) {
    if (threadIdx.x == 0) {
        double w_hat[3], a_hat[3];
        const double dt = hnet_ekf::imu_interval_inputs(S.s, r0, r1, pr.imu_avg != 0, w_hat, a_hat);
        hnet_ekf::propagate_jacobians_fill(S.s, pr.ext, dt, w_hat, F, Fw, pr.gravity_mag);
        hnet_ekf::propagate_mean(S.s, pr.ext, dt, w_hat, a_hat, pr.gravity_mag);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < NE; e += FILTER_THREADS) {                  // T = F P
        const int i = e / NS, j = e % NS;
        double a = 0.0;
        for (int q = 0; q < NS; q++) a += F[i * NS + q] * S.s.cov[q * NS + j];
        T[e] = a;
    }
    __syncthreads();
    double o[EPT];
    for (int r = 0; r < EPT; r++) {                                             // T F^T + Fw diag(q) Fw^T
        const int e = threadIdx.x + r * FILTER_THREADS;
        if (e < NE) {                                                           // (not `break`: in a function that form costs 130 registers)
            const int i = e / NS, j = e % NS;
            double a = 0.0;
            for (int q = 0; q < NS; q++) a += T[i * NS + q] * F[j * NS + q];
            for (int q = 0; q < NW; q++) a += Fw[i * NW + q] * pr.q[q] * Fw[j * NW + q];
            o[r] = a;
        }
    }
    for (int r = 0; r < EPT; r++) {
        const int e = threadIdx.x + r * FILTER_THREADS;
        if (e < NE) S.s.cov[e] = o[r];
    }
    __syncthreads();
}

}  // namespace

// IMU propagation of one listed session per workgroup over its selected readings (hnet_ekf::propagate_with_imu's loop), one cov_interval per pair of
// readings.  The result goes to work[b].
// ADV = false (hnet_filters_step): session ids[b], readings rd[rd_off[b] .. rd_off[b + 1]) selected on the host, time t_frame[b].
// ADV = true (hnet_filters_advance): session job[b].id, readings rd + b * 2 * (cap + 2) + (cap + 2) .. + res[b].n_sel from filter_select_kernel; the state
// comes from state[id] or, after the initialiser, from work[b]; a session the initialiser refused is skipped, one initialised after its frame keeps the
// initial state; job.reset: State::reset_4pt_offset afterwards (a session with fewer than two images: no forward follows).
template <bool ADV>
__global__ __launch_bounds__(FILTER_THREADS) void filter_propagate_kernel(const int32_t* __restrict__ ids, int n_sessions, const FilterRec* __restrict__ state,
                                                                          const FilterParams* __restrict__ params, const hnet_ekf::ImuData* __restrict__ rd,
                                                                          const int32_t* __restrict__ rd_off, const double* __restrict__ t_frame,
                                                                          FilterRec* work, const AdvanceJob* __restrict__ job, int cap,
                                                                          const AdvanceResult* __restrict__ res) {
    __shared__ FilterRec S;
    __shared__ double F[NE], Fw[NS * NW], T[NE];
    const int b = blockIdx.x, id = ADV ? job[b].id : ids[b];
    if (id < 0 || id >= n_sessions) return;                   // (host-validated)
    const FilterParams& pr = params[id];
    int k0, k1;
    if constexpr (ADV) {
        const AdvanceResult r = res[b];
        if (job[b].init && !r.ok) return;                      // (uniform over the workgroup, as the returns below)
        if (r.n_sel < 0 || r.n_sel > cap + 2) return;
        copy_rec(S, job[b].init ? work[b] : state[id]);
        k0 = 0;
        k1 = r.n_sel;
        rd += (size_t)b * 2 * (cap + 2) + (cap + 2);
    } else {
        copy_rec(S, state[id]);
        k0 = rd_off[b], k1 = rd_off[b + 1];
    }
    clear_jacobians(F, Fw);
    __syncthreads();
    if constexpr (ADV)
        if (job[b].init && S.t > job[b].t_frame) return;       // VioManager.cpp:203-206: work[b] holds the initial state
    for (int k = k0; k + 1 < k1; k++) cov_interval(S, pr, rd[k], rd[k + 1], F, Fw, T);
    if constexpr (ADV)
        if (job[b].reset) reset_offset_block(S);
    if (threadIdx.x == 0) S.t = ADV ? job[b].t_frame : t_frame[b];
    __syncthreads();
    copy_rec(work[b], S);
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
    copy_rec(S, work[b]);
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
        const bool singular = invert8_lanes(A, V);
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
    if (last) {
        reset_offset_block(S);
        __syncthreads();
    }
    copy_rec(work[b], S);
}

// the step's result work[b] -> state[ids[b]] (after the host accepted the step's forwards)
__global__ __launch_bounds__(FILTER_THREADS) void filter_scatter_kernel(const FilterRec* __restrict__ work, const int32_t* __restrict__ ids, int n_sessions,
                                                                        FilterRec* __restrict__ state) {
    const int b = blockIdx.x, id = ids[b];
    if (id < 0 || id >= n_sessions) return;
    copy_rec(state[id], work[b]);
}

// ---- the IMU feed and the cold start (hnet_filters_feed_imu / hnet_filters_advance) ----

namespace {
__device__ inline const hnet_ekf::ImuData& ring_at(const hnet_ekf::ImuData* rg, int head, int cap, int j) { return rg[(head + j) % cap]; }
// a session's ring is usable when its meta is consistent (the host wrote it; checked again because the kernels index with it)
__device__ inline bool ring_ok(const ImuRingMeta& m, int cap) { return m.head >= 0 && m.head < cap && m.count >= 0 && m.count <= cap; }

// The span of a session's ring rg (meta m: ring_ok and count >= 1, checked by the caller) that hnet_ekf::select_imu_readings can touch for the window
// [t0, t1], copied in time order into lin [cap + 2], by a workgroup of THREADS.  All lanes count the readings more than 10 s behind the newest (never
// used: hnet_ekf::trim_imu_prop), those before the window's start and those up to its end into the three LDS counters cnt (integers: the order of the
// atomics changes nothing); hnet_ekf::select_span turns the counts into the span, which is checked against the ring before anything is indexed with
// it and copied out (it may wrap).  -> its length, 0 when there is nothing usable.  Contains barriers: every call is uniform over the workgroup; lin
// is published on return.
template <int THREADS>
__device__ inline int ring_span(const hnet_ekf::ImuData* rg, const ImuRingMeta m, int cap, double t0, double t1, int* cnt, hnet_ekf::ImuData* lin) {
    const int t = threadIdx.x;
    const double newest = ring_at(rg, m.head, cap, m.count - 1).t;
    if (t < 3) cnt[t] = 0;
    __syncthreads();
    int c_old = 0, c_lt = 0, c_le = 0;
    for (int j = t; j < m.count; j += THREADS) {
        const double tt = ring_at(rg, m.head, cap, j).t;
        if (newest - tt > 10) c_old++;
        else { c_lt += tt < t0 ? 1 : 0; c_le += tt <= t1 ? 1 : 0; }
    }
    if (c_old) atomicAdd(&cnt[0], c_old);
    if (c_lt) atomicAdd(&cnt[1], c_lt);
    if (c_le) atomicAdd(&cnt[2], c_le);
    __syncthreads();
    int first = 0;
    int len = hnet_ekf::select_span(m.count - cnt[0], cnt[1], cnt[2], &first);
    if (len < 1 || len > cap || first < 0 || cnt[0] + first + len > m.count) len = 0;
    for (int k = t; k < len; k += THREADS) lin[k] = ring_at(rg, m.head, cap, cnt[0] + first + k);
    __syncthreads();
    return len;
}
}  // namespace

// feed: segment blockIdx.y's readings fed[src0 .. src0 + n) -> ring positions (wpos + k) % cap of session id; one lane records the ring's new head / count
__global__ __launch_bounds__(256) void imu_append_kernel(const ImuFeedSeg* __restrict__ seg, int n_fed, const hnet_ekf::ImuData* __restrict__ fed, int n_sessions,
                                                         int cap, hnet_ekf::ImuData* __restrict__ ring, ImuRingMeta* __restrict__ meta) {
    const ImuFeedSeg g = seg[blockIdx.y];
    if (g.id < 0 || g.id >= n_sessions || g.n < 0 || g.n > cap || g.wpos < 0 || g.wpos >= cap || g.src0 < 0 || g.src0 + g.n > n_fed) return;   // (host-validated)
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < g.n) ring[(size_t)g.id * cap + (g.wpos + k) % cap] = fed[g.src0 + k];
    if (k == 0 && g.head >= 0 && g.head < cap && g.count >= 0 && g.count <= cap) meta[g.id] = ImuRingMeta{g.head, g.count};
}

// The initialiser (hnet_ekf::initialize_with_imu + initialize_cov) for the listed sessions with job.init, one workgroup each, on the ring's readings
// not older than three windows behind the newest (hnet_ekf::trim_imu_init).  The window sums are reductions: every lane adds its readings (every
// 256th, in time order), then a fixed tree over the lanes; the decision and the mean come from the header's init_decide / init_from_stats on lane 0.
// Accepted: work[b] = {time0, mean, zero offsets, initialize_cov}, res[b] = {time0, ok 1}; refused: res[b].ok = 0 and work[b] is not written.
__global__ __launch_bounds__(FILTER_THREADS) void filter_init_kernel(const AdvanceJob* __restrict__ job, int n_sessions, int cap, const hnet_ekf::ImuData* __restrict__ ring,
                                                                     const ImuRingMeta* __restrict__ meta, const InitParams* __restrict__ ip,
                                                                     const FilterParams* __restrict__ params, FilterRec* __restrict__ work,
                                                                     AdvanceResult* __restrict__ res) {
    __shared__ FilterRec S;
    __shared__ double red[9][FILTER_THREADS];
    __shared__ int cnt[4];
    const int b = blockIdx.x, t = threadIdx.x;
    const AdvanceJob jb = job[b];
    if (!jb.init) return;
    const int id = jb.id;
    if (id < 0 || id >= n_sessions) return;
    const ImuRingMeta m = meta[id];
    const hnet_ekf::ImuData* rg = ring + (size_t)id * cap;
    const InitParams P = ip[id];
    const double w = P.window_time;
    bool refuse = !ring_ok(m, cap) || m.count < 2;                          // (uniform over the workgroup, as every test below)
    double newest = 0.0;
    int c3 = 0;
    if (!refuse) {
        newest = ring_at(rg, m.head, cap, m.count - 1).t;
        if (t < 4) cnt[t] = 0;
        __syncthreads();
        int c = 0;
        for (int j = t; j < m.count; j += FILTER_THREADS) c += ring_at(rg, m.head, cap, j).t < newest - 3 * w ? 1 : 0;   // trim_imu_init (time order: a prefix)
        if (c) atomicAdd(&cnt[0], c);
        __syncthreads();
        c3 = cnt[0];
        refuse = m.count - c3 < 2 || newest - ring_at(rg, m.head, cap, c3).t < 2 * w;
    }
    int n1 = 0, n2 = 0, last2 = -1;
    double avg[9];                                                           // a_avg_1to0, a_avg_2to1, w_avg_2to1
    if (!refuse) {
        double a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        int c1 = 0, c2 = 0, l2 = -1;
        for (int j = c3 + t; j < m.count; j += FILTER_THREADS) {
            const hnet_ekf::ImuData& d = ring_at(rg, m.head, cap, j);
            if (d.t > newest - 1 * w && d.t <= newest - 0 * w) {
                for (int i = 0; i < 3; i++) a[i] += d.am[i];
                c1++;
            }
            if (d.t > newest - 2 * w && d.t <= newest - 1 * w) {
                for (int i = 0; i < 3; i++) { a[3 + i] += d.am[i]; a[6 + i] += d.wm[i]; }
                c2++;
                l2 = j;
            }
        }
        for (int i = 0; i < 9; i++) red[i][t] = a[i];
        if (c1) atomicAdd(&cnt[1], c1);
        if (c2) atomicAdd(&cnt[2], c2);
        if (l2 >= 0) atomicMax(&cnt[3], l2 + 1);
        __syncthreads();
        for (int st = FILTER_THREADS / 2; st > 0; st >>= 1) {
            if (t < st)
                for (int i = 0; i < 9; i++) red[i][t] += red[i][t + st];
            __syncthreads();
        }
        n1 = cnt[1]; n2 = cnt[2]; last2 = cnt[3] - 1;
        refuse = n1 == 0 || n2 == 0;
        if (!refuse) {
            for (int i = 0; i < 3; i++) { avg[i] = red[i][0] / n1; avg[3 + i] = red[3 + i][0] / n2; avg[6 + i] = red[6 + i][0] / n2; }
        }
        __syncthreads();
    }
    if (!refuse) {
        double v1 = 0.0, v2 = 0.0;
        for (int j = c3 + t; j < m.count; j += FILTER_THREADS) {
            const hnet_ekf::ImuData& d = ring_at(rg, m.head, cap, j);
            if (d.t > newest - 1 * w && d.t <= newest - 0 * w) {
                const double e[3] = {d.am[0] - avg[0], d.am[1] - avg[1], d.am[2] - avg[2]};
                v1 += hnet_ekf::m3::dot(e, e);
            }
            if (d.t > newest - 2 * w && d.t <= newest - 1 * w) {
                const double e[3] = {d.am[0] - avg[3], d.am[1] - avg[4], d.am[2] - avg[5]};
                v2 += hnet_ekf::m3::dot(e, e);
            }
        }
        red[0][t] = v1;
        red[1][t] = v2;
        __syncthreads();
        for (int st = FILTER_THREADS / 2; st > 0; st >>= 1) {
            if (t < st) { red[0][t] += red[0][t + st]; red[1][t] += red[1][t + st]; }
            __syncthreads();
        }
        const double d1 = sqrt(red[0][0] / (n1 - 1)), d2 = sqrt(red[1][0] / (n2 - 1));        // (one reading: 0 / 0 = NaN, hnet_ekf::init_decide)
        refuse = !hnet_ekf::init_decide(d1, d2, P.imu_thresh, P.wait_for_jerk != 0);
    }
    if (refuse) {
        if (t == 0) res[b] = AdvanceResult{0.0, 0, 0};
        return;
    }
    double* sd = reinterpret_cast<double*>(&S);
    for (int i = t; i < FILTER_REC_DOUBLES; i += FILTER_THREADS) sd[i] = 0.0;        // a new State: zero offsets, zero covariance (State.cpp:79)
    __syncthreads();
    if (t == 0) {
        hnet_ekf::init_from_stats(avg + 3, avg + 6, P.init_height, params[id].gravity_mag, S.s);
        hnet_ekf::initialize_cov(S.s);
        S.t = ring_at(rg, m.head, cap, last2).t;
        res[b] = AdvanceResult{S.t, 1, 0};
    }
    __syncthreads();
    copy_rec(work[b], S);
}

// Selection (hnet_ekf::select_imu_readings) for the listed sessions straight from the ring, one workgroup each: window [state t, t_frame] + cam_imu_dt,
// the state's time read from state[id] (work[b] after the initialiser).  ring_span copies the span the header's loop can touch out of the ring and lane 0
// runs the header's function on it.
// sel + b * 2 * (cap + 2): the span [cap + 2], then the selected readings [cap + 2]; res[b].n_sel their number.
__global__ __launch_bounds__(FILTER_THREADS) void filter_select_kernel(const AdvanceJob* __restrict__ job, int n_sessions, int cap, const hnet_ekf::ImuData* __restrict__ ring,
                                                                       const ImuRingMeta* __restrict__ meta, const FilterRec* __restrict__ state,
                                                                       const FilterRec* __restrict__ work, hnet_ekf::ImuData* __restrict__ sel,
                                                                       AdvanceResult* __restrict__ res) {
    __shared__ int cnt[3];
    const int b = blockIdx.x, t = threadIdx.x;
    const AdvanceJob jb = job[b];
    const int id = jb.id;
    if (id < 0 || id >= n_sessions) return;
    if (jb.init && !res[b].ok) return;                                       // refused by the initialiser (n_sel is 0 already)
    if (!jb.init && t == 0) { res[b].time0 = 0.0; res[b].ok = 1; res[b].n_sel = 0; }
    const double t_state = jb.init ? work[b].t : state[id].t;
    if (!(jb.t_frame > t_state)) return;                                     // initialised later than this frame (VioManager.cpp:203-206) or at it: nothing to select
    const ImuRingMeta m = meta[id];
    if (!ring_ok(m, cap) || m.count < 1) return;
    const double t0 = t_state + jb.cam_imu_dt, t1 = jb.t_frame + jb.cam_imu_dt;
    hnet_ekf::ImuData* lin = sel + (size_t)b * 2 * (cap + 2);
    hnet_ekf::ImuData* out = lin + (cap + 2);
    const int len = ring_span<FILTER_THREADS>(ring + (size_t)id * cap, m, cap, t0, t1, cnt, lin);    // (every return above is uniform over the workgroup)
    if (len == 0) return;
    if (t == 0) res[b].n_sel = hnet_ekf::select_imu_readings(lin, len, t0, t1, out);          // writes at most len + 2 readings
}

// filter_scatter_kernel for hnet_filters_advance: work[b] -> state[id] unless the initialiser refused the session
__global__ __launch_bounds__(FILTER_THREADS) void filter_scatter_ok_kernel(const FilterRec* __restrict__ work, const AdvanceJob* __restrict__ job,
                                                                           const AdvanceResult* __restrict__ res, int n_sessions, FilterRec* __restrict__ state) {
    const int b = blockIdx.x, id = job[b].id;
    if (id < 0 || id >= n_sessions || !res[b].ok) return;
    copy_rec(state[id], work[b]);
}

// ---- prediction between frames (hnet_filters_predict) ----

namespace {
constexpr int REC_MEAN_DOUBLES = 29;                                          // t, then p q v ba bg offset: everything of a FilterRec before cov
static_assert(offsetof(FilterRec, s) + offsetof(hnet_ekf::State, cov) == REC_MEAN_DOUBLES * sizeof(double), "t and the mean are the record's first 29 doubles");

// what the reference's publishers form from the mean s at camera time t (hnet_ekf::odometry_from_state + prior_pixels) and the interval count, into the
// LDS record R; one lane
__device__ inline void predict_record(const hnet_ekf::State& s, double t, double cam_imu_dt, int intervals, PredictOut& R) {
    hnet_ekf::odometry_from_state(s, t, cam_imu_dt, R.o);
    double prior_cam[8];
    hnet_ekf::prior_pixels(s, R.prior_px, prior_cam);
    R.intervals = intervals;
}
}  // namespace

// The mean of each listed session at job[b].t_query and what the reference's publishers form from it (hnet_ekf::propagate_mean_with_imu +
// odometry_from_state + prior_pixels), one wavefront per session: the chain of mean updates is serial, the parallelism is across the sessions.  Of
// state[id] only t and the mean are read: S has room for the covariance only because propagate_mean takes a State&, S.s.cov is never loaded and
// nothing here may read it.  ring_span copies the span out of the ring, as for filter_select_kernel; lane 0 then runs the header's selection and mean
// loop on it and forms the record (predict_record).  Reads state / ring / meta / params, writes out[b] and scratch + b * 2 * (cap + 2) (the span
// [cap + 2], then the selection [cap + 2]) only.  A job the host refused (NO_STATE / WAIT_IMU) gets a zero
// record with that status, as does a ring the kernel finds empty or inconsistent (WAIT_IMU); t_query <= the state's t gives the state as it is
// (AT_STATE, 0 intervals).
__global__ __launch_bounds__(PREDICT_THREADS) void filter_predict_kernel(const PredictJob* __restrict__ job, int n_sessions, int cap,
                                                                         const hnet_ekf::ImuData* __restrict__ ring, const ImuRingMeta* __restrict__ meta,
                                                                         const FilterRec* __restrict__ state, const FilterParams* __restrict__ params,
                                                                         hnet_ekf::ImuData* __restrict__ scratch, PredictOut* __restrict__ out) {
    __shared__ FilterRec S;
    __shared__ PredictOut R;
    __shared__ int cnt[3];
    const int b = blockIdx.x, t = threadIdx.x;
    const PredictJob jb = job[b];
    const int id = jb.id;
    double* rw = reinterpret_cast<double*>(&R);
    for (int i = t; i < PREDICT_OUT_DOUBLES; i += PREDICT_THREADS) rw[i] = 0.0;          // (all-zero bits: intervals and status too)
    __syncthreads();
    int status = (id >= 0 && id < n_sessions) ? jb.status : PRED_NO_STATE;                // (host-validated; uniform over the workgroup, as every test below)
    if (status == PRED_OK) {
        const double* src = reinterpret_cast<const double*>(state + id);
        double* dst = reinterpret_cast<double*>(&S);
        for (int i = t; i < REC_MEAN_DOUBLES; i += PREDICT_THREADS) dst[i] = src[i];
        __syncthreads();
        const double t_state = S.t;
        hnet_ekf::ImuData* lin = scratch + (size_t)b * 2 * (cap + 2);
        int len = 0;
        if (!(jb.t_query > t_state)) status = PRED_AT_STATE;
        else {
            const ImuRingMeta m = meta[id];
            if (!ring_ok(m, cap) || m.count < 1) status = PRED_WAIT_IMU;          // (the host's mirror says so first: an empty ring has no reading past the query)
            else len = ring_span<PREDICT_THREADS>(ring + (size_t)id * cap, m, cap, t_state + jb.cam_imu_dt, jb.t_query + jb.cam_imu_dt, cnt, lin);
        }
        if (t == 0 && status != PRED_WAIT_IMU) {
            const FilterParams& pr = params[id];
            int done = 0;
            if (status == PRED_OK)                                                      // the selection writes at most len + 2 readings
                done = hnet_ekf::propagate_mean_with_imu(S.s, pr.ext, t_state, jb.t_query, lin, len, pr.gravity_mag, pr.imu_avg != 0, jb.cam_imu_dt, lin + (cap + 2));
            predict_record(S.s, status == PRED_OK ? jb.t_query : t_state, jb.cam_imu_dt, done, R);
        }
    }
    if (t == 0) R.status = status;
    __syncthreads();
    double* ow = reinterpret_cast<double*>(out + b);
    for (int i = t; i < PREDICT_OUT_DOUBLES; i += PREDICT_THREADS) ow[i] = rw[i];
}

// ---- prediction between frames with the covariance (hnet_filters_predict_cov) ----

// filter_predict_kernel's record plus the covariance at the query time, one workgroup of FILTER_THREADS per listed session; read-only.
// The status rules are filter_predict_kernel's and ring_span copies the span; lane 0 runs the header's select_imu_readings on it.  The intervals are
// filter_propagate_kernel's: cov_interval's body, every operation in its order (restated, see there), so mean and covariance are the advance's bit
// for bit before its reset.  Then lane 0 forms the record as filter_predict_kernel does (predict_record) and the 6 x 6 pose Jacobian; the derived
// blocks of hnet_ekf::odometry_cov_from_state go one element per lane through the header's element functions.  AT_STATE: the state's covariance as
// it is and its blocks; NO_STATE / WAIT_IMU: zero records and a zero row of `full`.  Reads state / ring / meta / params, writes out[b], cov_out[b],
// full + b * 729 (if given) and scratch + b * 2 * (cap + 2) only.
__global__ __launch_bounds__(FILTER_THREADS) void filter_predict_cov_kernel(const PredictJob* __restrict__ job, int n_sessions, int cap,
                                                                            const hnet_ekf::ImuData* __restrict__ ring, const ImuRingMeta* __restrict__ meta,
                                                                            const FilterRec* __restrict__ state, const FilterParams* __restrict__ params,
                                                                            hnet_ekf::ImuData* __restrict__ scratch, PredictOut* __restrict__ out,
                                                                            PredictCovOut* __restrict__ cov_out, double* __restrict__ full) {
    __shared__ FilterRec S;
    __shared__ double F[NE], Fw[NS * NW], T[NE];
    __shared__ PredictOut R;
    __shared__ double J[36], TJ[36];
    __shared__ int cnt[4];                                                              // ring_span's three counts, then the number of selected readings
    const int b = blockIdx.x, t = threadIdx.x;
    const PredictJob jb = job[b];
    const int id = jb.id;
    double* rw = reinterpret_cast<double*>(&R);
    for (int i = t; i < PREDICT_OUT_DOUBLES; i += FILTER_THREADS) rw[i] = 0.0;          // (all-zero bits: intervals and status too)
    clear_jacobians(F, Fw);
    __syncthreads();
    int status = (id >= 0 && id < n_sessions) ? jb.status : PRED_NO_STATE;              // (host-validated; uniform over the workgroup, as every test below)
    if (status == PRED_OK) {
        copy_rec(S, state[id]);
        __syncthreads();
        const FilterParams& pr = params[id];
        const double t_state = S.t;
        hnet_ekf::ImuData* lin = scratch + (size_t)b * 2 * (cap + 2);
        hnet_ekf::ImuData* rd = lin + (cap + 2);
        if (!(jb.t_query > t_state)) status = PRED_AT_STATE;
        else {
            const ImuRingMeta m = meta[id];
            if (!ring_ok(m, cap) || m.count < 1) status = PRED_WAIT_IMU;
            else {
                const double t0 = t_state + jb.cam_imu_dt, t1 = jb.t_query + jb.cam_imu_dt;
                const int len = ring_span<FILTER_THREADS>(ring + (size_t)id * cap, m, cap, t0, t1, cnt, lin);
                if (t == 0) cnt[3] = hnet_ekf::select_imu_readings(lin, len, t0, t1, rd);    // writes at most len + 2 readings
                __syncthreads();
            }
        }
        int done = 0;
        if (status == PRED_OK) {
            int n_sel = cnt[3];
            if (n_sel < 0 || n_sel > cap + 2) n_sel = 0;
            for (int k = 0; k + 1 < n_sel; k++) {                                        // cov_interval's body (F and Fw zeroed above)
                if (t == 0) {
                    double w_hat[3], a_hat[3];
                    const double dt = hnet_ekf::imu_interval_inputs(S.s, rd[k], rd[k + 1], pr.imu_avg != 0, w_hat, a_hat);
                    hnet_ekf::propagate_jacobians_fill(S.s, pr.ext, dt, w_hat, F, Fw, pr.gravity_mag);
                    hnet_ekf::propagate_mean(S.s, pr.ext, dt, w_hat, a_hat, pr.gravity_mag);
                }
                __syncthreads();
                for (int e = t; e < NE; e += FILTER_THREADS) {                           // T = F P
                    const int i = e / NS, j = e % NS;
                    double a = 0.0;
                    for (int q = 0; q < NS; q++) a += F[i * NS + q] * S.s.cov[q * NS + j];
                    T[e] = a;
                }
                __syncthreads();
                double o[EPT];
                for (int r = 0; r < EPT; r++) {                                          // T F^T + Fw diag(q) Fw^T
                    const int e = t + r * FILTER_THREADS;
                    if (e < NE) {
                        const int i = e / NS, j = e % NS;
                        double a = 0.0;
                        for (int q = 0; q < NS; q++) a += T[i * NS + q] * F[j * NS + q];
                        for (int q = 0; q < NW; q++) a += Fw[i * NW + q] * pr.q[q] * Fw[j * NW + q];
                        o[r] = a;
                    }
                }
                for (int r = 0; r < EPT; r++) {
                    const int e = t + r * FILTER_THREADS;
                    if (e < NE) S.s.cov[e] = o[r];
                }
                __syncthreads();
                done++;
            }
        }
        if (status != PRED_WAIT_IMU) {
            if (t == 0) {
                predict_record(S.s, status == PRED_OK ? jb.t_query : t_state, jb.cam_imu_dt, done, R);
                hnet_ekf::pose_cov_jacobian(S.s, J);
            }
            __syncthreads();
            if (t < 36) TJ[t] = hnet_ekf::pose_cov_left(J, S.s.cov, t / 6, t % 6);
        }
    }
    if (t == 0) R.status = status;
    __syncthreads();
    const bool live = status == PRED_OK || status == PRED_AT_STATE;
    double* ow = reinterpret_cast<double*>(out + b);
    for (int i = t; i < PREDICT_OUT_DOUBLES; i += FILTER_THREADS) ow[i] = rw[i];
    static_assert(PREDICT_COV_DOUBLES <= FILTER_THREADS && offsetof(hnet_ekf::OdometryCov, body_pos_cov) == 36 * sizeof(double) &&
                  offsetof(hnet_ekf::OdometryCov, body_vel_cov) == 45 * sizeof(double) && offsetof(hnet_ekf::OdometryCov, prior_cov_px) == 54 * sizeof(double),
                  "OdometryCov: pose 36, body position 9, body velocity 9, prior 64, one element per lane");
    if (t < PREDICT_COV_DOUBLES) {                                                       // hnet_ekf::odometry_cov_from_state, one element per lane
        double v = 0.0;
        if (live) {
            if (t < 36) v = hnet_ekf::pose_cov_elem(TJ, J, t / 6, t % 6);
            else if (t < 45) v = hnet_ekf::pose_cov_elem(TJ, J, hnet_ekf::frd_src((t - 36) / 3), hnet_ekf::frd_src((t - 36) % 3));
            else if (t < 54) v = hnet_ekf::body_vel_cov_elem(S.s.cov, (t - 45) / 3, (t - 45) % 3);
            else v = hnet_ekf::prior_cov_px_elem(S.s.cov, (t - 54) >> 3, (t - 54) & 7);
        }
        reinterpret_cast<double*>(cov_out + b)[t] = v;
    }
    if (full)
        for (int e = t; e < NE; e += FILTER_THREADS) full[(size_t)b * NE + e] = live ? S.s.cov[e] : 0.0;
}

// ---- innovation records and the NIS gate (hnet_filters_enable_innovations) ----

static_assert(offsetof(InnovRec, nis) == 16 * sizeof(double) && offsetof(InnovRec, iteration) == 17 * sizeof(double), "InnovRec: r, s_diag, nis, then the two ints");

// hnet_ekf::innovation for the measurement filter_update_kernel is about to apply in iteration `it`, one wavefront per listed session, and the gate
// rule of hnet_ekf::iterated_update_gated.  Of work[b] only the 64 covariance elements cov[sel(i)][sel(j)] are read.  S, r and the Gauss-Jordan inverse
// are the update kernel's (S and r formed as it forms them, the inverse by invert8_lanes); y = S^-1 r by lanes 0 .. 7 and the NIS as a
// serial sum in the header's order.  Flags: a session whose earlier update of this step found S singular (updates[b] < 0), or whose earlier record is
// REJECTED / SKIPPED, is SKIPPED; a closed reference gate otherwise gives NONE; both leave r, s_diag and nis zero.  A rejection writes 0 to gate[b],
// which is what makes filter_update_kernel skip this and the later updates and still do the last iteration's reset.  Writes innov[it * n + b] and
// gate[b] only.  PHOTO (a step with a photometric gate): verdict[b] != 0 says photo_gate_kernel refused the estimate of this or an earlier
// iteration, and the record is SKIPPED whatever the record before it says; without PHOTO the pointer is not read and the kernel is what it was.
template <bool PHOTO>
__global__ __launch_bounds__(INNOV_THREADS) void filter_innovation_kernel(const int32_t* __restrict__ ids, int n, int n_sessions, const FilterParams* __restrict__ params,
                                                                          const FilterRec* __restrict__ work, const float* __restrict__ net72,
                                                                          const double* __restrict__ prior_cam, const double* __restrict__ max_nis,
                                                                          int32_t* gate, const int32_t* __restrict__ updates, int it, InnovRec* innov,
                                                                          const int32_t* __restrict__ verdict) {
    __shared__ double A[64], V[64], r[8], sd[8], y[8];
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return;
    const int id = ids[b];
    if (id < 0 || id >= n_sessions) return;                                    // (host-validated; uniform over the workgroup, as every test below)
    InnovRec* out = innov + (size_t)it * n + b;
    double* ow = reinterpret_cast<double*>(out);
    int flag = hnet_ekf::INNOV_USED;
    if (updates[b] < 0) flag = hnet_ekf::INNOV_SKIPPED;
    else if (PHOTO && verdict[b] != 0) flag = hnet_ekf::INNOV_SKIPPED;
    else if (gate[b] == 0) {
        const int prev = it > 0 ? innov[(size_t)(it - 1) * n + b].flag : hnet_ekf::INNOV_NONE;
        flag = prev == hnet_ekf::INNOV_REJECTED || prev == hnet_ekf::INNOV_SKIPPED ? hnet_ekf::INNOV_SKIPPED : hnet_ekf::INNOV_NONE;
    }
    if (flag != hnet_ekf::INNOV_USED) {
        if (t < 17) ow[t] = 0.0;
        if (t == 0) { out->iteration = it; out->flag = flag; }
        return;
    }
    const double kc = params[id].k_net_cov;
    const float* nm = net72 + (size_t)b * 72;
    const int i = t >> 3, j = t & 7;
    A[t] = work[b].s.cov[sel(i) * NS + sel(j)] + kc * (double)nm[8 + t] / (hnet_ekf::F_PIX * hnet_ekf::F_PIX);
    V[t] = i == j ? 1.0 : 0.0;
    if (t < 8) r[t] = (double)nm[t] / hnet_ekf::F_PIX - prior_cam[(size_t)b * 8 + t];
    __syncthreads();
    if (t < 8) sd[t] = A[t * 9];
    const bool singular = invert8_lanes(A, V);
    double nis = (double)NAN;
    if (singular) flag = hnet_ekf::INNOV_SINGULAR;
    else {
        if (t < 8) {
            double a = 0.0;
            for (int q = 0; q < 8; q++) a += V[t * 8 + q] * r[q];
            y[t] = a;
        }
        __syncthreads();
        nis = 0.0;
        for (int q = 0; q < 8; q++) nis += r[q] * y[q];
        const double mx = max_nis[id];
        if (mx > 0.0 && nis > mx) flag = hnet_ekf::INNOV_REJECTED;               // (a NaN NIS does not reject)
    }
    __syncthreads();                                                           // (sd: a matrix singular in column 0 passed no barrier since it was written)
    if (t < 8) ow[t] = r[t];
    else if (t < 16) ow[t] = sd[t - 8];
    else if (t == 16) ow[16] = nis;
    if (t == 0) {
        out->iteration = it;
        out->flag = flag;
        if (flag == hnet_ekf::INNOV_REJECTED) gate[b] = 0;
    }
}

hipError_t launch_filter_innovation(const int32_t* ids, int n, int n_sessions, const FilterParams* params, const FilterRec* work, const float* net72,
                                    const double* prior_cam, const double* max_nis, int32_t* gate, const int32_t* updates, int it, InnovRec* innov,
                                    const int32_t* photo_verdict, hipStream_t s) {
    if (n < 1 || it < 0) return hipErrorInvalidValue;
    if (photo_verdict)
        hipLaunchKernelGGL(filter_innovation_kernel<true>, dim3((unsigned)n), dim3(INNOV_THREADS), 0, s, ids, n, n_sessions, params, work, net72, prior_cam, max_nis,
                           gate, updates, it, innov, photo_verdict);
    else
        hipLaunchKernelGGL(filter_innovation_kernel<false>, dim3((unsigned)n), dim3(INNOV_THREADS), 0, s, ids, n, n_sessions, params, work, net72, prior_cam, max_nis,
                           gate, updates, it, innov, photo_verdict);
    return hipGetLastError();
}

hipError_t launch_filter_predict(const PredictJob* job, int n, int n_sessions, int cap, const hnet_ekf::ImuData* ring, const ImuRingMeta* meta,
                                 const FilterRec* state, const FilterParams* params, hnet_ekf::ImuData* scratch, PredictOut* out, hipStream_t s) {
    if (n < 1 || cap < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_predict_kernel, dim3((unsigned)n), dim3(PREDICT_THREADS), 0, s, job, n_sessions, cap, ring, meta, state, params, scratch, out);
    return hipGetLastError();
}

hipError_t launch_filter_predict_cov(const PredictJob* job, int n, int n_sessions, int cap, const hnet_ekf::ImuData* ring, const ImuRingMeta* meta,
                                     const FilterRec* state, const FilterParams* params, hnet_ekf::ImuData* scratch, PredictOut* out,
                                     PredictCovOut* cov_out, double* full, hipStream_t s) {
    if (n < 1 || cap < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_predict_cov_kernel, dim3((unsigned)n), dim3(FILTER_THREADS), 0, s, job, n_sessions, cap, ring, meta, state, params, scratch, out,
                       cov_out, full);
    return hipGetLastError();
}

hipError_t launch_filter_propagate(const int32_t* ids, int n, int n_sessions, const FilterRec* state, const FilterParams* params, const hnet_ekf::ImuData* rd,
                                   const int32_t* rd_off, const double* t_frame, FilterRec* work, hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_propagate_kernel<false>, dim3((unsigned)n), dim3(FILTER_THREADS), 0, s, ids, n_sessions, state, params, rd, rd_off, t_frame, work,
                       (const AdvanceJob*)nullptr, 0, (const AdvanceResult*)nullptr);
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

hipError_t launch_imu_append(const ImuFeedSeg* seg, int n_seg, int max_seg_len, const hnet_ekf::ImuData* fed, int n_fed, int n_sessions, int cap,
                             hnet_ekf::ImuData* ring, ImuRingMeta* meta, hipStream_t s) {
    if (n_seg < 1 || n_seg > 65535 || max_seg_len < 1 || cap < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(imu_append_kernel, dim3((unsigned)((max_seg_len + 255) / 256), (unsigned)n_seg), dim3(256), 0, s, seg, n_fed, fed, n_sessions, cap, ring, meta);
    return hipGetLastError();
}

hipError_t launch_filter_init(const AdvanceJob* job, int n, int n_sessions, int cap, const hnet_ekf::ImuData* ring, const ImuRingMeta* meta, const InitParams* ip,
                              const FilterParams* params, FilterRec* work, AdvanceResult* res, hipStream_t s) {
    if (n < 1 || cap < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_init_kernel, dim3((unsigned)n), dim3(FILTER_THREADS), 0, s, job, n_sessions, cap, ring, meta, ip, params, work, res);
    return hipGetLastError();
}

hipError_t launch_filter_select(const AdvanceJob* job, int n, int n_sessions, int cap, const hnet_ekf::ImuData* ring, const ImuRingMeta* meta,
                                const FilterRec* state, const FilterRec* work, hnet_ekf::ImuData* sel, AdvanceResult* res, hipStream_t s) {
    if (n < 1 || cap < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_select_kernel, dim3((unsigned)n), dim3(FILTER_THREADS), 0, s, job, n_sessions, cap, ring, meta, state, work, sel, res);
    return hipGetLastError();
}

hipError_t launch_filter_propagate_adv(const AdvanceJob* job, int n, int n_sessions, int cap, const FilterRec* state, const FilterParams* params,
                                       const hnet_ekf::ImuData* sel, const AdvanceResult* res, FilterRec* work, hipStream_t s) {
    if (n < 1 || cap < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_propagate_kernel<true>, dim3((unsigned)n), dim3(FILTER_THREADS), 0, s, (const int32_t*)nullptr, n_sessions, state, params, sel,
                       (const int32_t*)nullptr, (const double*)nullptr, work, job, cap, res);
    return hipGetLastError();
}

hipError_t launch_filter_scatter_ok(const FilterRec* work, const AdvanceJob* job, const AdvanceResult* res, int n, int n_sessions, FilterRec* state, hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_scatter_ok_kernel, dim3((unsigned)n), dim3(FILTER_THREADS), 0, s, work, job, res, n_sessions, state);
    return hipGetLastError();
}

}  // namespace hnet
