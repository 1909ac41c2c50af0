// kernels_photo_search_oriented.hip — the device side of the coarse search under a table of orientation hypotheses (include/hnet.h
// hnet_op_photo_search_oriented, hnet_sessions_photo_search_oriented).  The oriented relocalisation
// (hnet_sessions_keyframe_relocalise_oriented) runs these two kernels between the per-slot kernels of kernels_photo_search.hip.
//
// photo_search_oriented_kernel: one workgroup of 256 threads per (entry, template, image) job.  The template thumbnail goes to LDS, the workgroup warps it
// there by the entry's integer matrix (hnet_search_oriented::warp_pixel) into template bytes and mask bytes: no launch of its own and no trip through
// global memory.  The image sits between 7r's two zeroed guards.  Thread t takes shifts t, t + 256, ...: 7r's scheme with the mask, per row of the overlap
// and group of four pixels one dword of the template, one of the mask, two of the image joined at the shift's byte offset, and six packed-u8 dot
// products (7r's five and n): n from the mask, Sb = dot(q, m), Sbb = dot(q & 255 m, q); Sa, Saa and Sab as in 7r, the warped template being zero where
// masked.  Integer sums: whatever the grouping, they are the host reference's.  The score is hnet_search::shift_score; the entry's best and second and
// its record are photo_search_kernel_dev.h's search_finish, the tail 7r's kernel runs.
// 256 threads and not 7r's 1024: with n_hyp times the workgroups the launch is bound by throughput, and 28 KB of LDS per workgroup lets five of them
// share a compute unit (20 wavefronts) where 1024 threads and 37 KB allow two.
// photo_search_winner_kernel: one wavefront per (template, image) pair, lane h holds entry h's best; the winner and the runner-up under
// hnet_search_oriented::hyp_better by a butterfly of lane exchanges (a total order: every lane ends with the same answer), lane 0 writes the record.
// This file is built with -ffp-contract=off.
// No atomics, no scratch, nothing waits on another workgroup; every table index, id, slot and candidate index is tested against its bound.
#include "photo_search_oriented_dev.h"
#include "photo_search_kernel_dev.h"

namespace hnet {

namespace ps = hnet_search;
namespace po = hnet_search_oriented;

namespace {
constexpr int PO_THREADS = 256;
static_assert(sizeof(SearchRec) % 4 == 0 && sizeof(OrientedRec) % 4 == 0 && sizeof(OrientedRec) / 4 <= 64, "a wavefront zeroes a search record in one step");

// hnet_search_oriented::shift_sums on the dwords in LDS: a_w the warped template [TWORDS], m_w its mask (bytes 1 / 0), b_w the image behind its guard
__device__ __forceinline__ void shift_sums_masked(const uint32_t* a_w, const uint32_t* m_w, const uint32_t* b_w, int dx, int dy, ps::Sums& s) {
    int u0, u1, v0, v1;
    ps::overlap(dx, dy, u0, u1, v0, v1);
    const int g0 = u0 >> 2, g1 = (u1 - 1) >> 2;
    const uint32_t mlo = 0xFFFFFFFFu << (8 * (u0 & 3)), mhi = 0xFFFFFFFFu >> (8 * (3 - ((u1 - 1) & 3)));      // the bytes of groups g0 and g1 inside the overlap
    const uint32_t sh = (uint32_t)(dx & 3);                               // (4 g + dx) mod 4, also for dx < 0
    uint32_t n = 0, sa = 0, sb = 0, sab = 0, saa = 0, sbb = 0;
    for (int v = v0; v < v1; v++) {
        const int bbase = PS_GUARD + (v + dy) * ps::TW + dx;              // byte of the image under template column 0: >= PS_GUARD - MAX_RX
        for (int g = g0; g <= g1; g++) {
            uint32_t e = 0xFFFFFFFFu;
            if (g == g0) e &= mlo;
            if (g == g1) e &= mhi;
            const int wi = (bbase + 4 * g) >> 2;
            const uint32_t p = a_w[v * ROW_WORDS + g] & e, m = m_w[v * ROW_WORDS + g] & e;
            const uint32_t q = __builtin_amdgcn_alignbyte(b_w[wi + 1], b_w[wi], sh);
            n = __builtin_amdgcn_udot4(m, 0x01010101u, n, false);
            sa = __builtin_amdgcn_udot4(p, 0x01010101u, sa, false);
            sb = __builtin_amdgcn_udot4(q, m, sb, false);
            sab = __builtin_amdgcn_udot4(p, q, sab, false);
            saa = __builtin_amdgcn_udot4(p, p, saa, false);
            sbb = __builtin_amdgcn_udot4(q & ((m << 8) - m), q, sbb, false);  // (255 m without a quarter-rate multiply: bytes of 1 or 0 become 255 or 0)
        }
    }
    s.n = (int32_t)n; s.sa = (int32_t)sa; s.sb = (int32_t)sb; s.sab = (int32_t)sab; s.saa = (int32_t)saa; s.sbb = (int32_t)sbb;
}

// the better of a lane's entry and every other lane's: hnet_search_oriented::offer_hyp is associative and commutative, so every lane returns the same
__device__ __forceinline__ po::BestHyp wave_best(po::BestHyp b) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double os = __shfl_xor(b.score, off, 64);
        const int oi = __shfl_xor(b.index, off, 64);
        po::offer_hyp(b, os, oi);
    }
    return b;
}
}  // namespace

// grid (n_hyp, jobs_x, n)
__global__ __launch_bounds__(PO_THREADS) void photo_search_oriented_kernel(const uint8_t* __restrict__ thumbs, int ta_stride, int tb_stride, int tb_off,
                                                                           const int32_t* __restrict__ valid, SearchOpts o, const SearchHyp* __restrict__ hyps,
                                                                           int n_hyp, SearchRec* __restrict__ hrec, double* __restrict__ scores) {
    __shared__ __attribute__((aligned(16))) uint32_t t_w[TWORDS];
    __shared__ __attribute__((aligned(16))) uint32_t a_w[TWORDS];
    __shared__ __attribute__((aligned(16))) uint32_t m_w[TWORDS];
    __shared__ __attribute__((aligned(16))) uint32_t b_w[BWORDS];
    __shared__ double sc[ps::NSHIFT];
    __shared__ double red_s[PO_THREADS];
    __shared__ int32_t red_i[PO_THREADS];
    const int tid = threadIdx.x, h = blockIdx.x, job = blockIdx.z * gridDim.y + blockIdx.y;
    if (n_hyp < 1 || n_hyp > po::MAX_HYP || h >= n_hyp) return;          // (workgroup-uniform, as is the next)
    if (valid && valid[job] == 0) return;
    const size_t slot = (size_t)job * n_hyp + h;
    {
        const uint32_t* ta = reinterpret_cast<const uint32_t*>(thumbs + ((size_t)blockIdx.z * ta_stride + blockIdx.y) * ps::TPIX);
        const uint32_t* tb = reinterpret_cast<const uint32_t*>(thumbs + ((size_t)blockIdx.z * tb_stride + tb_off) * ps::TPIX);
        for (int i = tid; i < TWORDS; i += PO_THREADS) t_w[i] = ta[i];
        for (int i = tid; i < BWORDS; i += PO_THREADS) b_w[i] = i >= PS_GUARD / 4 && i < PS_GUARD / 4 + TWORDS ? tb[i - PS_GUARD / 4] : 0u;
    }
    __syncthreads();
    {
        const int32_t b[4] = {hyps[h].b[0], hyps[h].b[1], hyps[h].b[2], hyps[h].b[3]};
        const uint8_t* t = reinterpret_cast<const uint8_t*>(t_w);
        uint8_t *a = reinterpret_cast<uint8_t*>(a_w), *m = reinterpret_cast<uint8_t*>(m_w);
        for (int i = tid; i < ps::TPIX; i += PO_THREADS) {               // warp_pixel reads t only inside the thumbnail, whatever b holds
            const int v = i / ps::TW, u = i - v * ps::TW;
            uint8_t val;
            m[i] = (uint8_t)po::warp_pixel(t, b, u, v, val);
            a[i] = val;
        }
    }
    __syncthreads();
    for (int i = tid; i < ps::NSHIFT; i += PO_THREADS) {
        int dx, dy;
        ps::index_shift(i, dx, dy);
        double v = ps::quiet_nan_d(), x;
        if (dx >= -o.radius_x && dx <= o.radius_x && dy >= -o.radius_y && dy <= o.radius_y) {
            ps::Sums s;
            shift_sums_masked(a_w, m_w, b_w, dx, dy, s);
            if (ps::shift_score(s, o.min_overlap, x)) v = x;
        }
        sc[i] = v;
    }
    __syncthreads();
    search_finish<PO_THREADS>(sc, red_s, red_i, o, [&](int dx, int dy, ps::Sums& s) { shift_sums_masked(a_w, m_w, b_w, dx, dy, s); }, slot, hrec, scores);
}

// grid (jobs)
__global__ __launch_bounds__(KEY_THREADS) void photo_search_winner_kernel(const SearchRec* __restrict__ hrec, const SearchHyp* __restrict__ hyps, int n_hyp, int jobs,
                                                                          const int32_t* __restrict__ valid, OrientedRec* __restrict__ out) {
    const int job = blockIdx.x, lane = threadIdx.x;
    if (job >= jobs || n_hyp < 1 || n_hyp > po::MAX_HYP) return;
    if (valid && valid[job] == 0) {                                       // (wavefront-uniform): not searched
        if (lane < (int)(sizeof(OrientedRec) / 4)) reinterpret_cast<uint32_t*>(out + job)[lane] = 0u;
        return;
    }
    const SearchRec* ph = hrec + (size_t)job * n_hyp;
    const bool scored = lane < n_hyp && po::hyp_scored(ph[lane]);
    po::BestHyp mine, win, second;
    po::hyp_none(mine);
    if (scored) po::offer_hyp(mine, ph[lane].score, lane);
    win = wave_best(mine);
    if (lane == win.index) po::hyp_none(mine);
    second = wave_best(mine);
    const int n_scored = __popcll(__ballot(scored));
    if (lane == 0) po::finish(ph, hyps, n_hyp, win, second, n_scored, out[job]);
}

hipError_t launch_photo_search_oriented(const uint8_t* thumbs, int ta_stride, int tb_stride, int tb_off, int jobs_x, int n, const int32_t* valid,
                                        const SearchOpts& opts, const SearchHyp* hyps, int n_hyp, SearchRec* hrec, double* scores, hipStream_t s) {
    if (n < 1 || n > 65535 || jobs_x < 1 || jobs_x > RELOC_MAX_CANDIDATES || ta_stride < 1 || tb_stride < 1 || tb_off < 0 || !thumbs || !hrec || !hyps ||
        n_hyp < 1 || n_hyp > SEARCH_MAX_HYP || (((uintptr_t)thumbs) & 3) || !ps::opts_valid(opts))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(photo_search_oriented_kernel, dim3((unsigned)n_hyp, (unsigned)jobs_x, (unsigned)n), dim3(PO_THREADS), 0, s, thumbs, ta_stride, tb_stride, tb_off,
                       valid, opts, hyps, n_hyp, hrec, scores);
    return hipGetLastError();
}

hipError_t launch_photo_search_winner(const SearchRec* hrec, const SearchHyp* hyps, int n_hyp, int jobs, const int32_t* valid, OrientedRec* out, hipStream_t s) {
    if (jobs < 1 || !hrec || !hyps || !out || n_hyp < 1 || n_hyp > SEARCH_MAX_HYP) return hipErrorInvalidValue;
    hipLaunchKernelGGL(photo_search_winner_kernel, dim3((unsigned)jobs), dim3(KEY_THREADS), 0, s, hrec, hyps, n_hyp, jobs, valid, out);
    return hipGetLastError();
}

}  // namespace hnet
