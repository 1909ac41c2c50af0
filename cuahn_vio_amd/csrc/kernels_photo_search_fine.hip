// kernels_photo_search_fine.hip — the device side of the fine stage of the search around the oriented winner (include/hnet.h hnet_op_photo_search_fine,
// hnet_sessions_photo_search_fine, hnet_sessions_keyframe_relocalise_fine).  The rule is include/hnet_photo_search_fine.h.
//
// photo_fine_thumbs_kernel: one thread per level-2 thumbnail pixel runs hnet_search_fine::thumb_pixel's cascade on its 4 x 4 block of the frame: level 2 of
// 7m's pyramid bit for bit, 4 480 bytes per frame.
// photo_search_fine_kernel: one workgroup of 512 threads per (fine entry, job).  It reads the job's coarse record and returns at once unless the record is
// FOUND, its winner lies inside the table and the job's candidate exists.  The level-2 template goes to LDS and is warped there by the entry's integer
// matrix into value bytes and mask bytes; the image sits between two zeroed guards of 68 bytes.  The work is the (shift, row) items: eight lanes share a
// shift, lane k of them takes rows v0 + k, v0 + k + 8, ... of the overlap, per group of four pixels one dword of the template, one of the mask, two of the
// image joined at the shift's byte offset (v_alignbyte_b32) and 7s's six packed-u8 dot products, byte masks at the two ends of a row.  The eight partial
// sums meet in a butterfly of lane exchanges: integers, so the order of the additions does not reach the bits.  64 shifts are in flight at once: the
// default radius 3 (49 shifts) is one pass, radius 4 (81) two.  One lane per shift scores it (hnet_search::shift_score) and keeps its sums in LDS, the
// first wavefront reduces the table under the header's total order, thread 0 writes the entry's best with the sums kept for it.
// 512 threads: the launch is a few hundred workgroups at most, fewer than two per compute unit, so what counts is the latency of ONE workgroup: the
// default's 392 (shift, row-class) lanes fit one pass.  20.2 KB of LDS and 8 wavefronts allow four workgroups per compute unit, which no launch reaches.
// Eight lanes of a shift read rows 80 bytes = 20 dwords apart: banks 0, 20, 8, 28, 16, 4, 24, 12 of the 32 of a ds_read_b32, and the four shifts of a
// 32-lane half differ by ex, i.e. by less than one dword: broadcasts or neighbouring banks.
// photo_search_fine_winner_kernel: one wavefront per job, lane j holds entry j's best; the best over the row by a butterfly under the same order (every
// lane ends with the same answer), lane 0 runs hnet_search_fine::finish.
// This file is built with -ffp-contract=off.  No atomics, no scratch, nothing waits on another workgroup; every index from a table or a record is tested
// against its bound before it is used.
#include "photo_search_fine_dev.h"

namespace hnet {

namespace ps = hnet_search;
namespace po = hnet_search_oriented;
namespace pf = hnet_search_fine;

namespace {
constexpr int PF_THREADS = 512, PF_SUB = 8, PF_AT_ONCE = PF_THREADS / PF_SUB;        // 64 shifts in flight
constexpr int PF_GUARD = 68;                                                          // guard bytes on either side of the image thumbnail in LDS
constexpr int FWORDS = pf::FPIX / 4, FROW_WORDS = pf::FW / 4, FBWORDS = (pf::FPIX + 2 * PF_GUARD) / 4;
constexpr int FTHUMB_BLOCKS = (pf::FPIX + 255) / 256;
static_assert(pf::FW % 4 == 0 && PF_GUARD % 4 == 0 && PF_GUARD >= pf::MAX_SX + 2, "rows are whole dwords; the guard holds the farthest column of a shifted group");
// the farthest dword a shift reads: row FH - 1, the last group of the row, shifted right by MAX_SX, and the dword after it
static_assert(((PF_GUARD + (pf::FH - 1) * pf::FW + pf::MAX_SX + (pf::FW - 4)) >> 2) + 1 < FBWORDS && PF_GUARD - pf::MAX_SX >= 0, "a shifted group stays inside the guards");
static_assert(PF_AT_ONCE == 64 && pf::NSHIFT <= 2 * 64 && sizeof(FineRec) % 4 == 0 && sizeof(OrientedRec) / 4 <= 64 && pf::MAX_FINE <= 64, "one wavefront reduces the table");

// the rows v0 + sub, v0 + sub + PF_SUB, ... of hnet_search_fine::shift_sums on the dwords in LDS: a_w the warped template [FWORDS], m_w its mask (bytes
// 1 / 0), b_w the image behind its guard
__device__ __forceinline__ void rows_sums(const uint32_t* a_w, const uint32_t* m_w, const uint32_t* b_w, int sx, int sy, int sub, uint32_t (&t)[6]) {
    int u0, u1, v0, v1;
    pf::overlap(sx, sy, u0, u1, v0, v1);
    const int g0 = u0 >> 2, g1 = (u1 - 1) >> 2;
    const uint32_t mlo = 0xFFFFFFFFu << (8 * (u0 & 3)), mhi = 0xFFFFFFFFu >> (8 * (3 - ((u1 - 1) & 3)));      // the bytes of groups g0 and g1 inside the overlap
    const uint32_t sh = (uint32_t)(sx & 3);                               // (4 g + sx) mod 4, also for sx < 0
    uint32_t n = 0, sa = 0, sb = 0, sab = 0, saa = 0, sbb = 0;
    for (int v = v0 + sub; v < v1; v += PF_SUB) {
        const int bbase = PF_GUARD + (v + sy) * pf::FW + sx;              // byte of the image under template column 0: >= PF_GUARD - MAX_SX
        for (int g = g0; g <= g1; g++) {
            uint32_t e = 0xFFFFFFFFu;
            if (g == g0) e &= mlo;
            if (g == g1) e &= mhi;
            const int wi = (bbase + 4 * g) >> 2;
            const uint32_t p = a_w[v * FROW_WORDS + g] & e, m = m_w[v * FROW_WORDS + g] & e;
            const uint32_t q = __builtin_amdgcn_alignbyte(b_w[wi + 1], b_w[wi], sh);
            n = __builtin_amdgcn_udot4(m, 0x01010101u, n, false);
            sa = __builtin_amdgcn_udot4(p, 0x01010101u, sa, false);
            sb = __builtin_amdgcn_udot4(q, m, sb, false);
            sab = __builtin_amdgcn_udot4(p, q, sab, false);
            saa = __builtin_amdgcn_udot4(p, p, saa, false);
            sbb = __builtin_amdgcn_udot4(q & ((m << 8) - m), q, sbb, false);  // (255 m: bytes of 1 or 0 become 255 or 0)
        }
    }
    t[0] = n; t[1] = sa; t[2] = sb; t[3] = sab; t[4] = saa; t[5] = sbb;
}

// the better of a lane's candidate and every other lane's: hnet_search_fine::offer is associative and commutative, so every lane returns the same
__device__ __forceinline__ pf::Best wave_best(pf::Best b) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double os = __shfl_xor(b.score, off, 64);
        const int oi = __shfl_xor(b.index, off, 64);
        pf::offer(b, os, oi);
    }
    return b;
}

// whether the fine stage runs on job `job`: the same test in the search and in the winner
__device__ __forceinline__ bool fine_runs(const OrientedRec& c, const int32_t* cand, int job, int n_hyp) {
    return (!cand || cand[job] >= 0) && pf::coarse_usable(c, n_hyp);
}
}  // namespace

// grid (blocks, count)
__global__ __launch_bounds__(256) void photo_fine_thumbs_kernel(const uint8_t* __restrict__ frames, const int32_t* __restrict__ idx, int n_frames,
                                                                uint8_t* __restrict__ thumbs) {
    const int pix = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    const int f = idx ? idx[i] : i;
    if (pix >= pf::FPIX || f < 0 || f >= n_frames) return;
    const int v = pix / pf::FW, u = pix - v * pf::FW;
    thumbs[(size_t)i * pf::FPIX + pix] = pf::thumb_pixel(frames + (size_t)f * NPIX, u, v);
}

// grid (n_fine, jobs)
__global__ __launch_bounds__(PF_THREADS) void photo_search_fine_kernel(const uint8_t* __restrict__ thumbs, int ta_stride, int tb_stride, int tb_off,
                                                                       const uint8_t* __restrict__ coarse, int coarse_stride, const int32_t* __restrict__ cand,
                                                                       int min_overlap, FineOpts fo, const SearchHyp* __restrict__ fine, int n_hyp,
                                                                       FineEntry* __restrict__ ent, double* __restrict__ scores) {
    __shared__ __attribute__((aligned(16))) uint32_t t_w[FWORDS];
    __shared__ __attribute__((aligned(16))) uint32_t a_w[FWORDS];
    __shared__ __attribute__((aligned(16))) uint32_t m_w[FWORDS];
    __shared__ __attribute__((aligned(16))) uint32_t b_w[FBWORDS];
    __shared__ double sc[pf::NSHIFT];
    __shared__ uint32_t sums[pf::NSHIFT][6];
    const int tid = threadIdx.x, j = blockIdx.x, job = blockIdx.y;
    if (!pf::opts_valid(fo) || j >= fo.n_fine || n_hyp < 1 || n_hyp > po::MAX_HYP) return;          // (workgroup-uniform, as is the next)
    const size_t slot = (size_t)job * fo.n_fine + j;
    const OrientedRec& c = *reinterpret_cast<const OrientedRec*>(coarse + (size_t)job * coarse_stride);
    if (!fine_runs(c, cand, job, n_hyp)) {
        if (scores)
            for (int i = tid; i < pf::NSHIFT; i += PF_THREADS) scores[slot * pf::NSHIFT + i] = ps::quiet_nan_d();
        return;
    }
    const int dx = c.base.dx, dy = c.base.dy;                             // |dx| <= 30, |dy| <= 20: coarse_usable
    const SearchHyp* hyp = fine + (size_t)c.hyp * fo.n_fine + j;         // c.hyp < n_hyp, j < n_fine
    {
        const uint32_t* ta = reinterpret_cast<const uint32_t*>(thumbs + (size_t)job * ta_stride * pf::FPIX);
        const uint32_t* tb = reinterpret_cast<const uint32_t*>(thumbs + ((size_t)job * tb_stride + tb_off) * pf::FPIX);
        for (int i = tid; i < FWORDS; i += PF_THREADS) t_w[i] = ta[i];
        for (int i = tid; i < FBWORDS; i += PF_THREADS) b_w[i] = i >= PF_GUARD / 4 && i < PF_GUARD / 4 + FWORDS ? tb[i - PF_GUARD / 4] : 0u;
    }
    __syncthreads();
    {
        const int32_t b[4] = {hyp->b[0], hyp->b[1], hyp->b[2], hyp->b[3]};
        const uint8_t* t = reinterpret_cast<const uint8_t*>(t_w);
        uint8_t *a = reinterpret_cast<uint8_t*>(a_w), *m = reinterpret_cast<uint8_t*>(m_w);
        for (int i = tid; i < pf::FPIX; i += PF_THREADS) {               // warp_pixel reads t only inside the thumbnail, whatever b holds
            const int v = i / pf::FW, u = i - v * pf::FW;
            uint8_t val;
            m[i] = (uint8_t)pf::warp_pixel(t, b, u, v, val);
            a[i] = val;
        }
    }
    __syncthreads();
    const int sub = tid & (PF_SUB - 1), lead = tid / PF_SUB;
    for (int base = 0; base < pf::NSHIFT; base += PF_AT_ONCE) {          // (every lane runs every pass: the exchanges below are among all lanes)
        const int i = base + lead;
        const int ey = i / pf::NE - pf::MAX_R, ex = i % pf::NE - pf::MAX_R;
        const bool in = i < pf::NSHIFT && ex >= -fo.radius && ex <= fo.radius && ey >= -fo.radius && ey <= fo.radius;
        uint32_t t[6] = {0, 0, 0, 0, 0, 0};
        if (in) rows_sums(a_w, m_w, b_w, 2 * dx + ex, 2 * dy + ey, sub, t);          // |2 dx + ex| <= 64, |2 dy + ey| <= 44
#pragma unroll
        for (int k = 0; k < 6; k++) {
#pragma unroll
            for (int off = PF_SUB / 2; off > 0; off >>= 1) t[k] += __shfl_xor(t[k], off, 64);
        }
        if (sub == 0 && i < pf::NSHIFT) {
            ps::Sums s;
            s.n = (int32_t)t[0]; s.sa = (int32_t)t[1]; s.sb = (int32_t)t[2]; s.sab = (int32_t)t[3]; s.saa = (int32_t)t[4]; s.sbb = (int32_t)t[5];
            double x;
            sc[i] = in && ps::shift_score(s, 4 * min_overlap, x) ? x : ps::quiet_nan_d();
#pragma unroll
            for (int k = 0; k < 6; k++) sums[i][k] = t[k];
        }
    }
    __syncthreads();
    if (tid < 64) {                                                       // the first wavefront: shifts tid and tid + 64
        pf::Best b;
        pf::best_none(b);
        pf::offer(b, sc[tid], j * pf::NSHIFT + tid);
        if (tid + 64 < pf::NSHIFT) pf::offer(b, sc[tid + 64], j * pf::NSHIFT + tid + 64);
        b = wave_best(b);
        if (tid == 0) {
            FineEntry e;
            e.score = b.score; e.index = b.index; e.pad = 0;
            e.s = ps::Sums{0, 0, 0, 0, 0, 0};
            const int k = b.index - j * pf::NSHIFT;
            if (b.index >= 0 && k >= 0 && k < pf::NSHIFT) {
                e.s.n = (int32_t)sums[k][0]; e.s.sa = (int32_t)sums[k][1]; e.s.sb = (int32_t)sums[k][2];
                e.s.sab = (int32_t)sums[k][3]; e.s.saa = (int32_t)sums[k][4]; e.s.sbb = (int32_t)sums[k][5];
            }
            ent[slot] = e;
        }
    }
    if (scores)
        for (int i = tid; i < pf::NSHIFT; i += PF_THREADS) scores[slot * pf::NSHIFT + i] = sc[i];
}

// grid (jobs)
__global__ __launch_bounds__(KEY_THREADS) void photo_search_fine_winner_kernel(const FineEntry* __restrict__ ent, int jobs, const uint8_t* __restrict__ coarse,
                                                                               int coarse_stride, const int32_t* __restrict__ cand, FineOpts fo,
                                                                               const SearchHyp* __restrict__ fine, int n_hyp, uint8_t* __restrict__ out, int out_stride,
                                                                               int part_off, int copy_coarse, float* __restrict__ x0) {
    const int job = blockIdx.x, lane = threadIdx.x;
    if (job >= jobs || !pf::opts_valid(fo) || n_hyp < 1 || n_hyp > po::MAX_HYP) return;
    const OrientedRec& c = *reinterpret_cast<const OrientedRec*>(coarse + (size_t)job * coarse_stride);
    uint8_t* o = out + (size_t)job * out_stride;
    if (copy_coarse && lane < (int)(sizeof(OrientedRec) / 4)) reinterpret_cast<uint32_t*>(o)[lane] = reinterpret_cast<const uint32_t*>(&c)[lane];
    const bool ran = fine_runs(c, cand, job, n_hyp);                      // (wavefront-uniform)
    pf::Best mine, best;
    pf::best_none(mine);
    ps::Sums s = {0, 0, 0, 0, 0, 0};
    if (ran && lane < fo.n_fine) {
        const FineEntry& e = ent[(size_t)job * fo.n_fine + lane];
        if (e.index >= lane * pf::NSHIFT && e.index < (lane + 1) * pf::NSHIFT) pf::offer(mine, e.score, e.index);
    }
    best = wave_best(mine);
    if (lane == 0) {
        const SearchHyp* row = ran ? fine + (size_t)c.hyp * fo.n_fine : nullptr;
        if (best.index >= 0) s = ent[(size_t)job * fo.n_fine + best.index / pf::NSHIFT].s;          // an index a lane offered: its own entry's
        FinePart& p = *reinterpret_cast<FinePart*>(o + part_off);
        pf::finish(c, row, fo.n_fine, ran, best, s, fo, p);
        if (x0 && p.flags != pf::FINE_SKIPPED)
            for (int k = 0; k < 8; k++) x0[(size_t)8 * job + k] = p.start_px[k];
    }
}

// grid (n)
__global__ __launch_bounds__(KEY_THREADS) void reloc_fine_pack_kernel(const OrientedRelocRec* __restrict__ base, int n, FineRelocRec* __restrict__ out) {
    const int b = blockIdx.x;
    if (b >= n) return;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(base + b);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&out[b].base);
    for (int i = threadIdx.x; i < (int)(sizeof(OrientedRelocRec) / 4); i += KEY_THREADS) dst[i] = src[i];
}

hipError_t launch_photo_fine_thumbs(const uint8_t* frames, const int32_t* idx, int n_frames, int count, uint8_t* thumbs, hipStream_t s) {
    if (count < 1 || count > 65535 || n_frames < 1 || !frames || !thumbs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(photo_fine_thumbs_kernel, dim3(FTHUMB_BLOCKS, (unsigned)count), dim3(256), 0, s, frames, idx, n_frames, thumbs);
    return hipGetLastError();
}

hipError_t launch_photo_search_fine(const uint8_t* thumbs, int ta_stride, int tb_stride, int tb_off, int jobs, const uint8_t* coarse, int coarse_stride,
                                    const int32_t* cand, const SearchOpts& opts, const FineOpts& fopts, const SearchHyp* fine, int n_hyp, FineEntry* ent,
                                    double* scores, hipStream_t s) {
    if (jobs < 1 || jobs > 65535 || ta_stride < 1 || tb_stride < 1 || tb_off < 0 || !thumbs || !coarse || !fine || !ent || n_hyp < 1 || n_hyp > SEARCH_MAX_HYP ||
        coarse_stride < (int)sizeof(OrientedRec) || (coarse_stride & 7) || (((uintptr_t)coarse) & 7) || (((uintptr_t)thumbs) & 3) || !ps::opts_valid(opts) ||
        !pf::opts_valid(fopts))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(photo_search_fine_kernel, dim3((unsigned)fopts.n_fine, (unsigned)jobs), dim3(PF_THREADS), 0, s, thumbs, ta_stride, tb_stride, tb_off, coarse,
                       coarse_stride, cand, opts.min_overlap, fopts, fine, n_hyp, ent, scores);
    return hipGetLastError();
}

hipError_t launch_photo_search_fine_winner(const FineEntry* ent, int jobs, const uint8_t* coarse, int coarse_stride, const int32_t* cand, const FineOpts& fopts,
                                           const SearchHyp* fine, int n_hyp, uint8_t* out, int out_stride, int part_off, bool copy_coarse, float* x0, hipStream_t s) {
    if (jobs < 1 || jobs > 65535 || !ent || !coarse || !fine || !out || n_hyp < 1 || n_hyp > SEARCH_MAX_HYP || coarse_stride < (int)sizeof(OrientedRec) ||
        (coarse_stride & 7) || (((uintptr_t)coarse) & 7) || (((uintptr_t)out) & 7) || (out_stride & 7) || (part_off & 7) || part_off < 0 ||
        out_stride < part_off + (int)sizeof(FinePart) || (copy_coarse && part_off < (int)sizeof(OrientedRec)) || !pf::opts_valid(fopts))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(photo_search_fine_winner_kernel, dim3((unsigned)jobs), dim3(KEY_THREADS), 0, s, ent, jobs, coarse, coarse_stride, cand, fopts, fine, n_hyp, out,
                       out_stride, part_off, copy_coarse ? 1 : 0, x0);
    return hipGetLastError();
}

hipError_t launch_reloc_fine_pack(const OrientedRelocRec* base, int n, FineRelocRec* out, hipStream_t s) {
    if (n < 1 || n > 65535 || !base || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(reloc_fine_pack_kernel, dim3((unsigned)n), dim3(KEY_THREADS), 0, s, base, n, out);
    return hipGetLastError();
}

}  // namespace hnet
