// kernels_photo_search.hip — the device side of the coarse search over integer translations (include/hnet.h hnet_op_photo_search,
// hnet_sessions_photo_search) and of the relocalisation of a session among its keyframes (hnet_sessions_keyframe_relocalise, its oriented
// form and the one inside hnet_sessions_keyframe_track_recover) around the unchanged launch_photo_align_robust.
//
// photo_thumbs_kernel / reloc_thumbs_kernel: one thread per thumbnail pixel reads its 8 x 8 block of the frame as eight 8-byte loads and runs
// hnet_search::thumb_pixel's cascade on it: level 3 of 7m's pyramid bit for bit, 1 120 bytes per frame, without the levels in between.
// photo_search_kernel: one workgroup of 1024 threads per (template, image) pair.  Both thumbnails sit in LDS as dwords (the image between two zeroed guards
// of 32 bytes, so that a group of four pixels may be read from any byte offset of any row of the overlap), the score of every shift of the range in LDS as
// doubles (20 008 bytes).  Thread t takes shifts t, t + 1024, t + 2048: per row of the overlap and group of four template pixels one dword of the template, two
// of the image joined at the shift's byte offset (v_alignbyte_b32), a byte mask at the two ends of the row, and five packed-u8 dot products
// (v_dot4_u32_u8) for Sa, Sb, Sab, Saa, Sbb.  Integer sums: whatever the grouping, they are the host reference's.  The score is
// hnet_search::shift_score.  The best and the second are two reductions of the table under the header's total order, a fixed tree through LDS
// (photo_search_kernel_dev.h, with the oriented kernel).
// The per-slot kernels of the relocalisation are one wavefront each, fp64 on lane 0, and this file is built with -ffp-contract=off like
// kernels_keyframe_map.hip: decide_relocalise and decide_revisit are the host reference's operations in its order.  The pick and the decision are
// templates over the call's record, instantiated here for the plain and for the oriented records.  The copy kernel moves 16-byte
// vectors.  No atomics, nothing waits on another workgroup, nothing spins; every id, slot and candidate index is tested against its table.
#include "photo_search_oriented_dev.h"
#include "photo_search_kernel_dev.h"

namespace hnet {

namespace kf = hnet_keyframe;
namespace km = hnet_keyframe_map;
namespace ps = hnet_search;
namespace rl = hnet_keyframe_reloc;

namespace {
constexpr int SV = NPIX / 16;                       // 16-byte vectors per frame
constexpr int SV_BLOCKS = (SV + 255) / 256;
constexpr int REC_DOUBLES = (int)(sizeof(RobustRec) / sizeof(double));
constexpr int THUMB_BLOCKS = (ps::TPIX + 255) / 256;                 // 5 workgroups of 256 threads per thumbnail
constexpr int PS_THREADS = 1024;
static_assert(sizeof(RobustRec) % sizeof(double) == 0 && offsetof(RelocRec, rv) == 0 && offsetof(OrientedRelocRec, rv) == 0 && offsetof(MapRevisit, rec) == 0 &&
              sizeof(RelocRec) % sizeof(double) == 0 && sizeof(SearchRec) % 4 == 0 && sizeof(OrientedRec) % 4 == 0, "the call's record: the alignment's first, as doubles");
static_assert(ps::STEP == 8 && ps::TW * ps::STEP == IMG_W && ps::TH * ps::STEP == IMG_H, "a thumbnail pixel is an 8 x 8 block of the frame");

// thumbnail pixel `pix` of the frame at src (8-byte aligned): the block's rows as 8-byte loads into a local 8 x 8 block, then the header's cascade on it
__device__ __forceinline__ uint8_t thumb_from_frame(const uint8_t* src, int pix) {
    const int v = pix / ps::TW, u = pix - v * ps::TW;
    uint32_t w[16];
    const uint8_t* p = src + (size_t)(ps::STEP * v) * IMG_W + ps::STEP * u;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const uint2 q = *reinterpret_cast<const uint2*>(p + r * IMG_W);
        w[2 * r] = q.x;
        w[2 * r + 1] = q.y;
    }
    // the cascade on dwords: byte k of row r is (w[2 r + (k >> 2)] >> 8 (k & 3)) & 255
    uint32_t l2[4];
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int i = 0; i < 2; i++) {
            uint32_t l1[4];
#pragma unroll
            for (int b = 0; b < 2; b++) {
                const uint32_t t = w[2 * (4 * j + 2 * b) + i], d = w[2 * (4 * j + 2 * b + 1) + i];      // four pixels of the upper and of the lower row
                l1[2 * b] = hnet_align::down4(t & 0xFFu, (t >> 8) & 0xFFu, d & 0xFFu, (d >> 8) & 0xFFu);
                l1[2 * b + 1] = hnet_align::down4((t >> 16) & 0xFFu, t >> 24, (d >> 16) & 0xFFu, d >> 24);
            }
            l2[2 * j + i] = hnet_align::down4(l1[0], l1[1], l1[2], l1[3]);
        }
    return hnet_align::down4(l2[0], l2[1], l2[2], l2[3]);
}

// hnet_search::shift_sums on the dwords in LDS: a_w the template [TWORDS], b_w the image behind its guard [BWORDS]
__device__ __forceinline__ void shift_sums_dot(const uint32_t* a_w, const uint32_t* b_w, int dx, int dy, ps::Sums& s) {
    int u0, u1, v0, v1;
    ps::overlap(dx, dy, u0, u1, v0, v1);
    const int g0 = u0 >> 2, g1 = (u1 - 1) >> 2;
    const uint32_t mlo = 0xFFFFFFFFu << (8 * (u0 & 3)), mhi = 0xFFFFFFFFu >> (8 * (3 - ((u1 - 1) & 3)));      // the bytes of groups g0 and g1 inside the overlap
    const uint32_t sh = (uint32_t)(dx & 3);                               // (4 g + dx) mod 4, also for dx < 0
    uint32_t sa = 0, sb = 0, sab = 0, saa = 0, sbb = 0;
    for (int v = v0; v < v1; v++) {
        const int bbase = PS_GUARD + (v + dy) * ps::TW + dx;              // byte of the image under template column 0: >= PS_GUARD - MAX_RX
        for (int g = g0; g <= g1; g++) {
            uint32_t m = 0xFFFFFFFFu;
            if (g == g0) m &= mlo;
            if (g == g1) m &= mhi;
            const int wi = (bbase + 4 * g) >> 2;
            const uint32_t p = a_w[v * ROW_WORDS + g] & m;
            const uint32_t q = __builtin_amdgcn_alignbyte(b_w[wi + 1], b_w[wi], sh) & m;
            sa = __builtin_amdgcn_udot4(p, 0x01010101u, sa, false);
            sb = __builtin_amdgcn_udot4(q, 0x01010101u, sb, false);
            sab = __builtin_amdgcn_udot4(p, q, sab, false);
            saa = __builtin_amdgcn_udot4(p, p, saa, false);
            sbb = __builtin_amdgcn_udot4(q, q, sbb, false);
        }
    }
    s.n = (u1 - u0) * (v1 - v0);
    s.sa = (int32_t)sa; s.sb = (int32_t)sb; s.sab = (int32_t)sab; s.saa = (int32_t)saa; s.sbb = (int32_t)sbb;
}

// the search part of a candidate's record: the pick compares plain and oriented records by it
__device__ __forceinline__ const SearchRec& search_part(const SearchRec& r) { return r; }
__device__ __forceinline__ const SearchRec& search_part(const OrientedRec& r) { return r.base; }
}  // namespace

// grid (THUMB_BLOCKS, count)
__global__ __launch_bounds__(256) void photo_thumbs_kernel(const uint8_t* __restrict__ frames, const int32_t* __restrict__ idx, int n_frames, uint8_t* __restrict__ thumbs) {
    const int pix = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    const int f = idx ? idx[i] : i;
    if (pix >= ps::TPIX || f < 0 || f >= n_frames) return;
    thumbs[(size_t)i * ps::TPIX + pix] = thumb_from_frame(frames + (size_t)f * NPIX, pix);
}

// grid (jobs_x, n)
__global__ __launch_bounds__(PS_THREADS) void photo_search_kernel(const uint8_t* __restrict__ thumbs, int ta_stride, int tb_stride, int tb_off,
                                                                  const int32_t* __restrict__ valid, SearchOpts o, SearchRec* __restrict__ rec,
                                                                  double* __restrict__ scores) {
    __shared__ __attribute__((aligned(16))) uint32_t a_w[TWORDS];
    __shared__ __attribute__((aligned(16))) uint32_t b_w[BWORDS];
    __shared__ double sc[ps::NSHIFT];
    __shared__ double red_s[PS_THREADS];
    __shared__ int32_t red_i[PS_THREADS];
    const int tid = threadIdx.x, job = blockIdx.y * gridDim.x + blockIdx.x;
    if (valid && valid[job] == 0) {                                       // (workgroup-uniform)
        if (tid < (int)(sizeof(SearchRec) / 4)) reinterpret_cast<uint32_t*>(rec + job)[tid] = 0u;
        if (scores)
            for (int i = tid; i < ps::NSHIFT; i += PS_THREADS) scores[(size_t)job * ps::NSHIFT + i] = ps::quiet_nan_d();
        return;
    }
    {
        const uint32_t* ta = reinterpret_cast<const uint32_t*>(thumbs + ((size_t)blockIdx.y * ta_stride + blockIdx.x) * ps::TPIX);
        const uint32_t* tb = reinterpret_cast<const uint32_t*>(thumbs + ((size_t)blockIdx.y * tb_stride + tb_off) * ps::TPIX);
        for (int i = tid; i < TWORDS; i += PS_THREADS) a_w[i] = ta[i];
        for (int i = tid; i < BWORDS; i += PS_THREADS) b_w[i] = i >= PS_GUARD / 4 && i < PS_GUARD / 4 + TWORDS ? tb[i - PS_GUARD / 4] : 0u;
    }
    __syncthreads();
    for (int i = tid; i < ps::NSHIFT; i += PS_THREADS) {
        int dx, dy;
        ps::index_shift(i, dx, dy);
        double v = ps::quiet_nan_d(), x;
        if (dx >= -o.radius_x && dx <= o.radius_x && dy >= -o.radius_y && dy <= o.radius_y) {
            ps::Sums s;
            shift_sums_dot(a_w, b_w, dx, dy, s);
            if (ps::shift_score(s, o.min_overlap, x)) v = x;
        }
        sc[i] = v;
    }
    __syncthreads();
    search_finish<PS_THREADS>(sc, red_s, red_i, o, [&](int dx, int dy, ps::Sums& s) { shift_sums_dot(a_w, b_w, dx, dy, s); }, (size_t)job, rec, scores);
}

// grid (THUMB_BLOCKS * (M + 2), n); active != nullptr: a slot with active[b] == 0 has no candidate
__global__ __launch_bounds__(256) void reloc_thumbs_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ slot, int n_sessions,
                                                           const int32_t* __restrict__ active, const KeyState* __restrict__ state, const uint8_t* __restrict__ key,
                                                           MapStore map, const uint8_t* __restrict__ ring, int n_slots, uint8_t* __restrict__ thumbs,
                                                           int32_t* __restrict__ valid) {
    const int M = reloc_map_ok(map) ? map.capacity : 0;
    const int j = blockIdx.x / THUMB_BLOCKS, pix = (blockIdx.x - j * THUMB_BLOCKS) * 256 + threadIdx.x, b = blockIdx.y;
    if (j > M + 1) return;                                                // (the grid is the host's M + 2)
    const int id = ids[b], sc = slot[b];
    const bool call_ok = (!active || active[b] != 0) && id >= 0 && id < n_sessions && id < map.n_sessions && sc >= 0 && sc < n_slots;
    const uint8_t* src = nullptr;
    if (call_ok) {
        if (j == 0) {
            if (state[id].has_key != 0) src = key + (size_t)id * NPIX;
        } else if (j <= M) {
            const int ms = j - 1;
            if (map.entry[(size_t)id * M + ms].valid != 0 && ms != map.state[id].cur_slot) src = map.img + ((size_t)id * M + ms) * NPIX;
        } else {
            src = ring + (size_t)sc * NPIX;
        }
    }
    if (j <= M && pix == 0) valid[(size_t)b * (M + 1) + j] = src ? 1 : 0;
    if (!src || pix >= ps::TPIX) return;
    thumbs[((size_t)b * (M + 2) + j) * ps::TPIX + pix] = thumb_from_frame(src, pix);
}

// SRec / Out: SearchRec / RelocRec, or OrientedRec / OrientedRelocRec
template <class SRec, class Out>
__global__ __launch_bounds__(KEY_THREADS) void reloc_pick_kernel(const int32_t* __restrict__ ids, int n, int n_sessions, const KeyState* __restrict__ state, int M,
                                                                 const int32_t* __restrict__ valid, const SRec* __restrict__ srec, float* __restrict__ x0,
                                                                 int32_t* __restrict__ cand, int32_t* __restrict__ mslot, Out* __restrict__ out) {
    static_assert(sizeof(out->search) == sizeof(SRec), "the record holds the pick's search record");
    const int b = blockIdx.x;
    if (b >= n || threadIdx.x != 0) return;
    const int id = ids[b];
    double hb[9];
    for (int k = 0; k < 9; k++) hb[k] = (k & 3) == 0 ? 1.0 : 0.0;
    rl::Pick p;
    rl::pick_none(p);
    int searched = 0, found = 0;
    if (id >= 0 && id < n_sessions && M >= 0 && M <= km::MAX_CAPACITY) {
        if (state[id].has_key != 0) km::origin_curr(state[id], hb);
        for (int c = 0; c <= M; c++) {
            if (valid[(size_t)b * (M + 1) + c] == 0) continue;
            const SearchRec& r = search_part(srec[(size_t)b * (M + 1) + c]);
            searched++;
            found += r.flags == ps::FOUND ? 1 : 0;
            rl::offer(p, c, r);
        }
    }
    const SRec* pick = p.index >= 0 ? srec + (size_t)b * (M + 1) + p.index : nullptr;
    uint32_t* so = reinterpret_cast<uint32_t*>(&out[b].search);
    const uint32_t* si = reinterpret_cast<const uint32_t*>(pick);
    for (int k = 0; k < (int)(sizeof(SRec) / 4); k++) so[k] = pick ? si[k] : 0u;
    for (int k = 0; k < 8; k++) x0[(size_t)b * 8 + k] = pick ? search_part(*pick).start_px[k] : kf::quiet_nan();
    cand[b] = p.index;
    mslot[b] = p.index >= 1 ? p.index - 1 : -1;
    out[b].target = rl::target_of(p.index);
    out[b].n_searched = searched;
    out[b].n_found = found;
    out[b].pad = 0;
    for (int k = 0; k < 9; k++) out[b].rv.h_origin_before[k] = hb[k];
}

__global__ __launch_bounds__(256) void reloc_gather_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ slot, int n_sessions,
                                                           const int32_t* __restrict__ cand, const uint4* __restrict__ key, const uint4* __restrict__ img, int capacity,
                                                           const uint4* __restrict__ ring, int n_slots, uint4* __restrict__ prev, uint4* __restrict__ curr) {
    const int v = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    const int c = cand[b];
    if (c < 0 || c > capacity) return;                                    // (capacity is 0 without a map: only the held keyframe)
    const int id = ids[b], sc = slot[b];
    if (v >= SV || id < 0 || id >= n_sessions || sc < 0 || sc >= n_slots) return;
    const uint4 p = c == 0 ? key[(size_t)id * SV + v] : img[((size_t)id * capacity + (c - 1)) * SV + v], q = ring[(size_t)sc * SV + v];
    prev[(size_t)b * SV + v] = p;
    curr[(size_t)b * SV + v] = q;
}

// Out: RelocRec or OrientedRelocRec
template <class Out>
__global__ __launch_bounds__(KEY_THREADS) void reloc_decide_kernel(const int32_t* __restrict__ ids, int n, int n_sessions, const RobustRec* __restrict__ rec,
                                                                   const float* x0, const int32_t* __restrict__ cand, RelocOpts opts, KeyState* state, MapStore map,
                                                                   Out* out, int32_t* __restrict__ attach) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return;
    const int id = ids[b];
    const int M = reloc_map_ok(map) ? map.capacity : 0;
    const bool valid = id >= 0 && id < n_sessions && id < map.n_sessions;
    int c = cand[b];
    if (!valid || c < 0 || c > M) c = -1;
    const double* src = reinterpret_cast<const double*>(rec + b);
    double* dst = reinterpret_cast<double*>(out + b);
    for (int i = t; i < REC_DOUBLES; i += KEY_THREADS) dst[i] = c >= 0 ? src[i] : 0.0;
    if (t != 0) return;
    MapRevisit& rv = out[b].rv;
    if (!valid) {
        for (int i = REC_DOUBLES; i < (int)(sizeof(MapRevisit) / sizeof(double)); i++) dst[i] = 0.0;
        rv.slot = -1;
        rv.flags = rl::RL_NO_CANDIDATE;
        attach[b] = 0;
        return;
    }
    if (c == 0) {
        rl::decide_relocalise(state[id], x0 + (size_t)b * 8, rv.h_origin_before, rec[b], opts, state[id], rv);
        attach[b] = 0;
        return;
    }
    MapOpts mo;
    rl::revisit_opts(opts, mo);
    if (M > 0) {
        const MapEntry* e = map.entry + (size_t)id * M;
        attach[b] = km::decide_revisit(state[id], map.state[id], c >= 1 ? e + (c - 1) : nullptr, c - 1, 0, x0 + (size_t)b * 8, rv.h_origin_before, rec[b], mo, state[id],
                                       map.state[id], rv);
    } else {                                                              // without a map only "no pick" arrives here
        MapState none = {-1, 0, 0, 0};
        attach[b] = km::decide_revisit(state[id], none, nullptr, -1, 0, x0 + (size_t)b * 8, rv.h_origin_before, rec[b], mo, state[id], none, rv);
    }
}

namespace {
bool bad_grid(int n) { return n < 1 || n > 65535; }

template <class SRec, class Out>
hipError_t reloc_pick(const int32_t* ids, int n, int n_sessions, const KeyState* state, int M, const int32_t* valid, const SRec* srec, float* x0, int32_t* cand,
                      int32_t* mslot, Out* out, hipStream_t s) {
    if (n < 1 || M < 0 || M > km::MAX_CAPACITY) return hipErrorInvalidValue;
    hipLaunchKernelGGL((reloc_pick_kernel<SRec, Out>), dim3((unsigned)n), dim3(KEY_THREADS), 0, s, ids, n, n_sessions, state, M, valid, srec, x0, cand, mslot, out);
    return hipGetLastError();
}

template <class Out>
hipError_t reloc_decide(const int32_t* ids, int n, int n_sessions, const RobustRec* rec, const float* x0, const int32_t* cand, const RelocOpts& opts, KeyState* state,
                        const MapStore& map, Out* out, int32_t* attach, hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL((reloc_decide_kernel<Out>), dim3((unsigned)n), dim3(KEY_THREADS), 0, s, ids, n, n_sessions, rec, x0, cand, opts, state, map, out, attach);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_photo_thumbs(const uint8_t* frames, const int32_t* idx, int n_frames, int count, uint8_t* thumbs, hipStream_t s) {
    if (bad_grid(count) || n_frames < 1 || !frames || !thumbs || (((uintptr_t)frames) & 7)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(photo_thumbs_kernel, dim3(THUMB_BLOCKS, (unsigned)count), dim3(256), 0, s, frames, idx, n_frames, thumbs);
    return hipGetLastError();
}

hipError_t launch_photo_search(const uint8_t* thumbs, int ta_stride, int tb_stride, int tb_off, int jobs_x, int n, const int32_t* valid, const SearchOpts& opts,
                               SearchRec* rec, double* scores, hipStream_t s) {
    if (bad_grid(n) || jobs_x < 1 || jobs_x > RELOC_MAX_CANDIDATES || ta_stride < 1 || tb_stride < 1 || tb_off < 0 || !thumbs || !rec || (((uintptr_t)thumbs) & 3) ||
        !ps::opts_valid(opts))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(photo_search_kernel, dim3((unsigned)jobs_x, (unsigned)n), dim3(PS_THREADS), 0, s, thumbs, ta_stride, tb_stride, tb_off, valid, opts, rec, scores);
    return hipGetLastError();
}

hipError_t launch_reloc_thumbs(const int32_t* ids, const int32_t* slot, int n, int n_sessions, const int32_t* active, const KeyState* state, const uint8_t* key,
                               const MapStore& map, const uint8_t* ring, int n_slots, uint8_t* thumbs, int32_t* valid, hipStream_t s) {
    const int M = map.img ? map.capacity : 0;
    if (bad_grid(n) || M < 0 || M > km::MAX_CAPACITY || ((((uintptr_t)key) | (uintptr_t)map.img | (uintptr_t)ring) & 7)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(reloc_thumbs_kernel, dim3((unsigned)(THUMB_BLOCKS * (M + 2)), (unsigned)n), dim3(256), 0, s, ids, slot, n_sessions, active, state, key, map,
                       ring, n_slots, thumbs, valid);
    return hipGetLastError();
}

hipError_t launch_reloc_pick(const int32_t* ids, int n, int n_sessions, const KeyState* state, int M, const int32_t* valid, const SearchRec* srec, float* x0,
                             int32_t* cand, int32_t* mslot, RelocRec* out, hipStream_t s) {
    return reloc_pick(ids, n, n_sessions, state, M, valid, srec, x0, cand, mslot, out, s);
}

hipError_t launch_reloc_pick(const int32_t* ids, int n, int n_sessions, const KeyState* state, int M, const int32_t* valid, const OrientedRec* srec, float* x0,
                             int32_t* cand, int32_t* mslot, OrientedRelocRec* out, hipStream_t s) {
    return reloc_pick(ids, n, n_sessions, state, M, valid, srec, x0, cand, mslot, out, s);
}

hipError_t launch_reloc_gather(const int32_t* ids, const int32_t* slot, int n, int n_sessions, const int32_t* cand, const uint8_t* key, const MapStore& map,
                               const uint8_t* ring, int n_slots, uint8_t* prev, uint8_t* curr, hipStream_t s) {
    const int M = map.img ? map.capacity : 0;
    if (bad_grid(n) || ((((uintptr_t)key) | (uintptr_t)map.img | (uintptr_t)ring | (uintptr_t)prev | (uintptr_t)curr) & 15)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(reloc_gather_kernel, dim3(SV_BLOCKS, (unsigned)n), dim3(256), 0, s, ids, slot, n_sessions, cand, (const uint4*)key, (const uint4*)map.img, M,
                       (const uint4*)ring, n_slots, (uint4*)prev, (uint4*)curr);
    return hipGetLastError();
}

hipError_t launch_reloc_decide(const int32_t* ids, int n, int n_sessions, const RobustRec* rec, const float* x0, const int32_t* cand, const RelocOpts& opts,
                               KeyState* state, const MapStore& map, RelocRec* out, int32_t* attach, hipStream_t s) {
    return reloc_decide(ids, n, n_sessions, rec, x0, cand, opts, state, map, out, attach, s);
}

hipError_t launch_reloc_decide(const int32_t* ids, int n, int n_sessions, const RobustRec* rec, const float* x0, const int32_t* cand, const RelocOpts& opts,
                               KeyState* state, const MapStore& map, OrientedRelocRec* out, int32_t* attach, hipStream_t s) {
    return reloc_decide(ids, n, n_sessions, rec, x0, cand, opts, state, map, out, attach, s);
}

}  // namespace hnet
