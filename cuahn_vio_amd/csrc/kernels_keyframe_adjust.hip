// kernels_keyframe_adjust.hip — the device side of the joint adjustment of a keyframe map (include/hnet.h hnet_op_keyframe_adjust_solve,
// hnet_op_keyframe_adjust, hnet_sessions_keyframe_adjust).  Three small launches around the unchanged launch_photo_align_robust - the pairs
// of a session's stored keyframes that overlap and the start of each (one wavefront per session, a lane per pair, the job list compacted with a ballot),
// a round of jobs gathered into the staging arrays, each job's level-0 record judged into its row of the session's edge table - and the SOLVE: one
// workgroup of 256 lanes per session runs build, the whole Levenberg-Marquardt loop and finish of include/hnet_keyframe_adjust.h with the session's
// Problem (the normal matrix, its factor, the per-edge Jacobian blocks and weights) in LDS.  The header's executor is the workgroup here: for_each spreads
// tasks over the lanes, single is lane 0, both between barriers; every task's sums are the header's in its order, so a record equals the host
// reference's byte for byte.  Built with -ffp-contract=off like the other keyframe objects.  No atomics, nothing waits on another workgroup.  The host
// side that enqueues these kernels is capi_keyframe_adjust.hip.
#include "keyframe_adjust_dev.h"

namespace hnet {

namespace kf = hnet_keyframe;
namespace km = hnet_keyframe_map;
namespace ka = hnet_adjust;

namespace {
constexpr int SV = NPIX / 16;                       // 16-byte vectors per frame
static_assert(NPIX % 16 == 0, "frames must stay 16-byte aligned in the map and the staging arrays");
constexpr int SV_BLOCKS = (SV + 255) / 256;
constexpr int REC_DOUBLES = (int)(sizeof(AdjustRec) / sizeof(double)), ALIGN_DOUBLES = (int)(sizeof(RobustRec) / sizeof(double));
static_assert(KEY_THREADS >= ADJUST_MAX_PAIRS && KEY_THREADS == ADJUST_INFO && offsetof(AdjustRec, n_pairs) == 8 && offsetof(AdjustRec, n_jobs) == 12 &&
              sizeof(RobustRec) % sizeof(double) == 0, "a lane per pair and per entry of an information matrix; n_pairs | n_jobs are double 1 of a record");

__device__ inline bool source_ok(const AdjustSource& src, int id) {
    return id >= 0 && id < src.n_sessions && src.capacity >= 1 && src.capacity <= ka::MAX_ENTRIES;
}

// job g of the call, numbered through the slots in order -> (b, k); false: there is no such job
__device__ inline bool locate(const AdjustJobs* tab, int n, int g, int& b, int& k) {
    int rest = g;
    for (b = 0; b < n; b++) {
        int c = tab[b].count;
        c = c < 0 ? 0 : c > ADJUST_MAX_PAIRS ? ADJUST_MAX_PAIRS : c;
        if (rest < c) { k = rest; return rest >= 0; }
        rest -= c;
    }
    b = k = 0;
    return false;
}

// the header's executor on one workgroup: a barrier on both sides of every step, so that what a step decides (Problem::stop, fail) is read by every lane
// between two steps and never while lane 0 writes it
struct Workgroup {
    int tid;
    template <class F> __device__ void for_each(int n, F f) {
        __syncthreads();
        for (int t = tid; t < n; t += ADJUST_THREADS) f(t);
        __syncthreads();
    }
    template <class F> __device__ void single(F f) {
        __syncthreads();
        if (tid == 0) f();
        __syncthreads();
    }
};
}  // namespace

__global__ __launch_bounds__(KEY_THREADS) void keyframe_adjust_pairs_kernel(const int32_t* __restrict__ ids, int n, AdjustSource src, int min_grid,
                                                                            AdjustJobs* __restrict__ tab, AdjustRec* __restrict__ rec) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return;
    const int id = ids[b];
    const bool valid = source_ok(src, id);                                 // (uniform over the wavefront)
    AdjustJob jb;
    ka::job_zero(jb);
    int kind = 0;
    if (valid && t < ADJUST_MAX_PAIRS) kind = ka::pair_job(src.entry + (size_t)id * src.capacity, src.capacity, t, min_grid, jb);
    const unsigned long long jobs = __ballot(kind == 2), prs = __ballot(kind >= 1);
    const int count = __popcll(jobs);
    // row t of the table is the job of the lane that holds the t-th set bit of the ballot: every lane writes its own row and no other
    unsigned long long rest = jobs;
    for (int r = 0; r < t && rest; r++) rest &= rest - 1ull;
    const int from = t < count ? __ffsll((long long)rest) - 1 : -1, lane = from < 0 ? 0 : from;
    AdjustJob row;
    row.i = __shfl(jb.i, lane);
    row.j = __shfl(jb.j, lane);
    row.grid = __shfl(jb.grid, lane);
    row.pad = 0;
    for (int k = 0; k < ka::NC; k++) row.start_px[k] = __shfl(jb.start_px[k], lane);
    if (from < 0) ka::job_zero(row);
    AdjustJobs& out = tab[b];
    if (t < ADJUST_MAX_PAIRS) out.job[t] = row;
    double* r = reinterpret_cast<double*>(rec + b);
    for (int i = t; i < REC_DOUBLES; i += KEY_THREADS)
        if (i != 1) r[i] = 0.0;                                            // (double 1 is n_pairs | n_jobs: lane 0's)
    if (t == 0) {
        out.count = count;
        out.n_pairs = __popcll(prs);
        rec[b].n_pairs = 0;
        rec[b].n_jobs = count;
    }
}

__global__ __launch_bounds__(256) void keyframe_adjust_gather_kernel(const int32_t* __restrict__ ids, int n, const uint4* __restrict__ img, int n_sessions, int capacity,
                                                                     const AdjustJobs* __restrict__ tab, int first, uint4* __restrict__ prev,
                                                                     uint4* __restrict__ curr, float* __restrict__ x0) {
    const int v = blockIdx.x * 256 + threadIdx.x, q = blockIdx.y;
    int b, k;
    bool ok = locate(tab, n, first + q, b, k);                             // (uniform over the workgroup)
    int id = 0, i = 0, j = 0;
    if (ok) {
        id = ids[b];
        i = tab[b].job[k].i;
        j = tab[b].job[k].j;
        ok = id >= 0 && id < n_sessions && i >= 0 && i < capacity && j >= 0 && j < capacity;
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) x0[(size_t)q * 8 + threadIdx.x] = ok ? tab[b].job[k].start_px[threadIdx.x] : kf::quiet_nan();
    if (!ok || v >= SV) return;
    const uint4 p = img[((size_t)id * capacity + i) * SV + v], c = img[((size_t)id * capacity + j) * SV + v];
    prev[(size_t)q * SV + v] = p;
    curr[(size_t)q * SV + v] = c;
}

__global__ __launch_bounds__(KEY_THREADS) void keyframe_adjust_edge_kernel(int n, const AdjustJobs* __restrict__ tab, int first, int n_round,
                                                                           const RobustRec* __restrict__ align_rec, AdjustOpts opts, AdjustRec* __restrict__ rec,
                                                                           double* __restrict__ infos, RobustRec* __restrict__ edge_recs) {
    const int q = blockIdx.x, t = threadIdx.x;
    if (q >= n_round) return;
    int b, k;
    if (!locate(tab, n, first + q, b, k)) return;
    const size_t row = (size_t)b * ADJUST_MAX_PAIRS + k;
    infos[row * ADJUST_INFO + t] = align_rec[q].px.info[t];
    if (edge_recs) {
        const double* src = reinterpret_cast<const double*>(align_rec + q);
        double* dst = reinterpret_cast<double*>(edge_recs + row);
        for (int i = t; i < ALIGN_DOUBLES; i += KEY_THREADS) dst[i] = src[i];
    }
    if (t == 0) ka::judge_edge(tab[b].job[k], align_rec[q], opts, rec[b].edge[k]);
}

__global__ __launch_bounds__(ADJUST_THREADS) void keyframe_adjust_solve_kernel(const int32_t* __restrict__ ids, int n, AdjustSource src, const double* infos,
                                                                               AdjustOpts opts, AdjustRec* rec) {
    __shared__ ka::Problem P;
    const int b = blockIdx.x;
    if (b >= n) return;
    Workgroup par{(int)threadIdx.x};
    const int id = ids[b];
    const bool valid = source_ok(src, id);                                 // (uniform over the workgroup)
    AdjustRec& out = rec[b];
    km::Entry* e = valid ? src.entry + (size_t)id * src.capacity : nullptr;
    const int m = valid ? src.capacity : 0;
    par.single([&] { ka::build(e, m, infos ? infos + (size_t)b * ADJUST_MAX_PAIRS * ADJUST_INFO : nullptr, opts, out, P); });
    if (P.flags == 0) ka::solve(P, opts, par);
    par.single([&] {
        ka::finish(P, opts, e, m, out);
        if (valid && src.state && src.mstate) ka::apply_state(out, opts, src.mstate[id], m, src.state[id]);
    });
}

namespace {
bool bad_grid(int n) { return n < 1 || n > 65535; }
bool unaligned(const void* a, const void* b = nullptr, const void* c = nullptr) { return ((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15; }
}  // namespace

hipError_t launch_keyframe_adjust_pairs(const int32_t* ids, int n, const AdjustSource& src, int min_grid, AdjustJobs* tab, AdjustRec* rec, hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyframe_adjust_pairs_kernel, dim3((unsigned)n), dim3(KEY_THREADS), 0, s, ids, n, src, min_grid, tab, rec);
    return hipGetLastError();
}

hipError_t launch_keyframe_adjust_gather(const int32_t* ids, int n, const AdjustSource& src, const AdjustJobs* tab, int first, int n_round, uint8_t* prev,
                                         uint8_t* curr, float* x0, hipStream_t s) {
    if (n < 1 || first < 0 || bad_grid(n_round) || unaligned(src.img, prev, curr)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyframe_adjust_gather_kernel, dim3(SV_BLOCKS, (unsigned)n_round), dim3(256), 0, s, ids, n, (const uint4*)src.img, src.n_sessions, src.capacity,
                       tab, first, (uint4*)prev, (uint4*)curr, x0);
    return hipGetLastError();
}

hipError_t launch_keyframe_adjust_edge(int n, const AdjustJobs* tab, int first, int n_round, const RobustRec* align_rec, const AdjustOpts& opts, AdjustRec* rec,
                                       double* infos, RobustRec* edge_recs, hipStream_t s) {
    if (n < 1 || first < 0 || n_round < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyframe_adjust_edge_kernel, dim3((unsigned)n_round), dim3(KEY_THREADS), 0, s, n, tab, first, n_round, align_rec, opts, rec, infos, edge_recs);
    return hipGetLastError();
}

hipError_t launch_keyframe_adjust_solve(const int32_t* ids, int n, const AdjustSource& src, const double* infos, const AdjustOpts& opts, AdjustRec* rec,
                                        hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyframe_adjust_solve_kernel, dim3((unsigned)n), dim3(ADJUST_THREADS), 0, s, ids, n, src, infos, opts, rec);
    return hipGetLastError();
}

}  // namespace hnet
