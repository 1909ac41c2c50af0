// kernels_photo.hip — photometric residual records (photo_dev.h, include/hnet.h hnet_photo_residual).
//
// For every frame pair and every candidate homography the kernel sums the reference's photometric error map
//   e(u, v) = |warp(img2, H)(u, v) - img1(u, v)| * 255          (model_to_trace.py:319-327)
// over the image instead of writing it: 24 bytes per (pair, candidate) leave the device, not 71 680.  The per-pixel value is errmap_kernel<uint8_t>'s
// expression on the same device functions (warp_coords, warp_taps_global, the exact u8 -> float conversion), so that every e has the bits of the existing
// error map for the same H.
//
// Form: one workgroup of 256 threads per (row slice, pair).  The pair's whole img2 (71 680 bytes) is staged once in LDS with 16-byte loads, so every tap of every
// candidate is an LDS byte read and any sampling position is covered: there is no fallback path.  Lanes c < m form the m matrices once per workgroup (dlt_solve
// in double, rounded to nine floats).  Candidate loop outside, pixel loop inside; a thread takes quads of 4 consecutive pixels (one 32-bit load of img1,
// coalesced), in ascending pixel order, and accumulates in double.  Lanes are reduced by a fixed __shfl_down tree, the 4 waves in wave order through LDS, the
// 7 slices in slice order by photo_finish_kernel: no floating-point atomics, and a pair's record depends on the pair alone.
//
// Departures from the recommended form, and why:
//  - the u8 -> float conversion is PixRead<uint8_t>::cvt (three VALU operations, bit-identical to the 256-entry table for all 256 bytes:
//    test_u8_scaling_is_exact) instead of a table in LDS: four more scattered LDS reads per sample would double the load on the LDS pipe, which the byte taps
//    already keep busy, while the VALU work spreads over the 4 SIMDs.
//  - the slice partials are added by a second, tiny launch instead of the slice that arrives last: the XCDs' L2 caches are not coherent with each other, so a
//    last-arriver needs system-scope stores, a ticket counter that must return to zero and a fence protocol, all for ~2 us on a diagnostic path.
//  - the filters' candidates are read where the step leaves them (PhotoCands) instead of being packed by a kernel of their own: one launch fewer.
//
// The photometric gate of the filters needs a step's records before the update they guard, one iteration at a time: photo_iter_kernel runs the
// same workgroup body (photo_slice_body) on the candidates of ONE iteration and photo_gate_kernel finishes them, forms the verdict and closes the gate.
#include "filters_dev.h"      // hnet_ekf::photo_reject for the device (photo_gate_kernel); first, so that the header is compiled host + device
#include "photo_dev.h"
#include "warp_dev.h"

namespace hnet {

namespace {
constexpr int PH_THREADS = 256, PH_WAVES = PH_THREADS / 64;
constexpr int PH_QUADS = PHOTO_SLICE_PIX / (4 * PH_THREADS);                  // 10 quads per thread and candidate
// dynamic LDS: img2 (staged forms only) | aux.  aux for a capacity of C candidates: H [C][9] f32 | flags [C] i32 | per-wave sums [C][4] f64 x 2 | per-wave counts [C][4] i32
constexpr int ph_aux_bytes(int cap) { return cap * (9 * 4 + 4 + 2 * PH_WAVES * 8 + PH_WAVES * 4); }
struct PhAux { float* hs; int* fl; double *w_sum, *w_sin; int* w_cnt; };
__device__ __forceinline__ PhAux ph_aux(uint8_t* base, int cap) {
    PhAux a;
    a.w_sum = reinterpret_cast<double*>(base);                                 // (the doubles first: 8-byte alignment for any capacity)
    a.w_sin = a.w_sum + cap * PH_WAVES;
    a.hs = reinterpret_cast<float*>(a.w_sin + cap * PH_WAVES);
    a.fl = reinterpret_cast<int*>(a.hs + cap * 9);
    a.w_cnt = a.fl + cap;
    return a;
}
constexpr int PH_LDS_BYTES = NPIX + ph_aux_bytes(PHOTO_MAX_CAND);             // 79 600: two workgroups per CU
constexpr int PH_ITER_CAND = 3;                                                // the per-iteration launch: {zero, prior, forward 0} or {forward it}
constexpr int PH_ITER_LDS_STAGED = NPIX + ph_aux_bytes(PH_ITER_CAND), PH_ITER_LDS_GLOBAL = ph_aux_bytes(PH_ITER_CAND);
static_assert(NPIX % 16 == 0, "the aux sections start 16-byte aligned behind img2");
static_assert(2 * PH_LDS_BYTES <= 160 * 1024, "two workgroups share a CU's LDS");
}  // namespace

// The work of one workgroup (row slice `slice` of pair `pair`) for the m candidates first .. first + m - 1 of a pair's `stride` candidates: candidate c's
// offsets as PhotoCands says for index first + c, its partial at partial[(pair * stride + first + c) * PHOTO_SLICES + slice].  STAGED: the pair's img2 goes
// to LDS (at lds, the aux sections behind it) and every tap is an LDS byte read; otherwise the taps are read from global memory through the same
// warp_taps_global and lds holds the aux sections only.  The arithmetic is the same either way: a record's bits depend on neither the form nor on which
// launch formed it.
template <bool STAGED>
__device__ __forceinline__ void photo_slice_body(const uint8_t* __restrict__ img1, const uint8_t* __restrict__ img2, const PhotoCands& cands, int m, int first,
                                                 int stride, int cap, PhotoRec* __restrict__ partial, float* __restrict__ map, uint8_t* lds, int pair, int slice) {
    const PhAux aux = ph_aux(lds + (STAGED ? NPIX : 0), cap);
    float* hs = aux.hs;
    int* fl = aux.fl;
    double *w_sum = aux.w_sum, *w_sin = aux.w_sin;
    int* w_cnt = aux.w_cnt;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* tile = img2 + (size_t)pair * NPIX;
    if (STAGED) {
        // img2 of the pair -> LDS, 16 bytes per lane
        const uint4* src = reinterpret_cast<const uint4*>(tile);
        for (int i = tid; i < NPIX / 16; i += PH_THREADS) reinterpret_cast<uint4*>(lds)[i] = src[i];
        tile = lds;
    }
    // the m matrices: H = (float) dlt_solve(p4 + offsets), the corners an fp32 sum as in dlt_kernel; a non-finite entry makes the whole matrix NaN, so that
    // every sampling position is NaN: every sample 0, no pixel inside
    if (tid < m) {
        const int cl = first + tid;
        const float* o = nullptr;
        if (cands.offsets) o = cands.offsets + ((size_t)pair * stride + cl) * 8;
        else if (cl == 1) o = cands.prior + (size_t)pair * 8;
        else if (cl >= 2) o = cands.net + (size_t)(cl - 2) * cands.net_iter_stride + (size_t)pair * 72;
        double d[8], h[9];
#pragma unroll
        for (int k = 0; k < 8; k++) d[k] = (double)(float)(p4(k) + (double)(o ? o[k] : 0.0f));
        dlt_solve(d, h);
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 9; k++) ok = ok && isfinite((float)h[k]);
#pragma unroll
        for (int k = 0; k < 9; k++) hs[tid * 9 + k] = ok ? (float)h[k] : __builtin_nanf("");
        fl[tid] = ok ? 0 : PHOTO_DEGENERATE;
    }
    __syncthreads();

    const uint8_t* a_img = img1 + (size_t)pair * NPIX;
    const int pix0 = slice * PHOTO_SLICE_PIX + 4 * tid;
    for (int c = 0; c < m; c++) {
        float h[9];
#pragma unroll
        for (int k = 0; k < 9; k++) h[k] = hs[c * 9 + k];
        float* mp = map ? map + ((size_t)pair * stride + first + c) * NPIX : nullptr;
        double s_all = 0.0, s_in = 0.0;
        int n_in = 0;
        for (int q = 0; q < PH_QUADS; q++) {
            const int pix = pix0 + q * (4 * PH_THREADS);
            const int v = pix / IMG_W, u0 = pix - v * IMG_W;
            const uint32_t a4 = *reinterpret_cast<const uint32_t*>(a_img + pix);
            float e4[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                float ix, iy, Z;
                warp_coords(h, u0 + j, v, ix, iy, Z);
                const float w = warp_taps_global<uint8_t, false>(tile, ix, iy, nullptr);
                const float e = fabsf(w - PixRead<uint8_t>::cvt((uint8_t)(a4 >> (8 * j)))) * 255.0f;
                const bool in = -0.5f < ix && ix < (float)IMG_W - 0.5f && -0.5f < iy && iy < (float)IMG_H - 0.5f;     // false for NaN
                s_all += (double)e;
                if (in) { s_in += (double)e; n_in++; }
                e4[j] = e;
            }
            if (mp) *reinterpret_cast<float4*>(mp + pix) = make_float4(e4[0], e4[1], e4[2], e4[3]);
        }
        s_all = wave_sum(s_all);
        s_in = wave_sum(s_in);
        n_in = wave_sum(n_in);
        if (lane == 0) {
            w_sum[c * PH_WAVES + wave] = s_all;
            w_sin[c * PH_WAVES + wave] = s_in;
            w_cnt[c * PH_WAVES + wave] = n_in;
        }
    }
    __syncthreads();
    if (tid < m) {
        PhotoRec r = {0.0, 0.0, 0, fl[tid]};
#pragma unroll
        for (int w = 0; w < PH_WAVES; w++) {
            r.sum += w_sum[tid * PH_WAVES + w];
            r.sum_inside += w_sin[tid * PH_WAVES + w];
            r.n_inside += w_cnt[tid * PH_WAVES + w];
        }
        partial[((size_t)pair * stride + first + tid) * PHOTO_SLICES + slice] = r;
    }
}

// grid: PHOTO_SLICES * n workgroups (slice = block % PHOTO_SLICES); partial [n][m][PHOTO_SLICES]
__global__ __launch_bounds__(PH_THREADS) void photo_residual_kernel(const uint8_t* __restrict__ img1, const uint8_t* __restrict__ img2, PhotoCands cands, int m,
                                                                    PhotoRec* __restrict__ partial, float* __restrict__ map) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ph_lds[];
    const int pair = blockIdx.x / PHOTO_SLICES, slice = blockIdx.x - pair * PHOTO_SLICES;
    photo_slice_body<true>(img1, img2, cands, m, 0, m, PHOTO_MAX_CAND, partial, map, ph_lds, pair, slice);
}

// The records of ONE iteration of a filters step (the photometric gate): of a pair's 2 + iters candidates the m from `first` on - {zero, prior of
// iteration 0, forward 0} for iteration 0 (first 0, m 3), {forward it} later (first 2 + it, m 1) - into the same partial [n][2 + iters][PHOTO_SLICES] the
// one launch after the last update would fill.  Same grid; cands.offsets is null.  M is a template parameter so that the two uses are two kernels with
// names of their own in a kernel trace.
template <bool STAGED, int M>
__global__ __launch_bounds__(PH_THREADS) void photo_iter_kernel(const uint8_t* __restrict__ img1, const uint8_t* __restrict__ img2, PhotoCands cands, int first,
                                                                int stride, PhotoRec* __restrict__ partial) {
    static_assert(M <= PH_ITER_CAND, "the aux sections hold PH_ITER_CAND candidates");
    extern __shared__ __attribute__((aligned(16))) uint8_t ph_lds[];
    const int pair = blockIdx.x / PHOTO_SLICES, slice = blockIdx.x - pair * PHOTO_SLICES;
    photo_slice_body<STAGED>(img1, img2, cands, M, first, stride, PH_ITER_CAND, partial, nullptr, ph_lds, pair, slice);
}

// record i = the sum of its slices' partials in slice order
__global__ __launch_bounds__(64) void photo_finish_kernel(const PhotoRec* __restrict__ partial, int count, PhotoRec* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    PhotoRec r = {0.0, 0.0, 0, 0};
#pragma unroll
    for (int s = 0; s < PHOTO_SLICES; s++) {
        const PhotoRec p = partial[(size_t)i * PHOTO_SLICES + s];
        r.sum += p.sum;
        r.sum_inside += p.sum_inside;
        r.n_inside += p.n_inside;
        r.flags |= p.flags;
    }
    out[i] = r;
}

static_assert(sizeof(hnet_ekf::PhotoRecord) == sizeof(PhotoRec) && offsetof(hnet_ekf::PhotoRecord, n_inside) == offsetof(PhotoRec, n_inside) &&
              (int)hnet_ekf::PHOTO_DEGENERATE == PHOTO_DEGENERATE && (int)hnet_ekf::PHOTO_REJECTED == PHOTO_REJECTED, "PhotoRec is the header's PhotoRecord");

// Iteration `it` of a gated step, between photo_iter_kernel and the innovation / update kernels; one lane per stepping session b.  Finishes the records
// photo_iter_kernel left partials for - candidates 0, 1, 2 at it == 0, candidate 2 + it later - as photo_finish_kernel does (the 7 slices in slice order) into
// the download's rec[b][2 + iters].  Then the verdict of hnet_ekf::iterated_update_photo_gated: formed iff the reference gate is still open (gate[b] != 0: no
// NIS or photometric rejection so far either, both close it), no update found S singular (updates[b] >= 0) and the slot has no verdict yet; on rejection
// the record takes PHOTO_REJECTED, gate[b] = 0 (filter_update_kernel then skips this and the later updates and still does the last iteration's reset) and
// verdict[b] = 1 + it (filter_innovation_kernel: SKIPPED from here on).  Iteration 0 writes verdict[b] for every slot, so that every attempt starts clean.
__global__ __launch_bounds__(64) void photo_gate_kernel(const PhotoRec* __restrict__ partial, int n, int it, int stride, const int32_t* __restrict__ ids,
                                                        int n_sessions, const PhotoGate* __restrict__ gates, const int32_t* __restrict__ updates, int32_t* gate,
                                                        int32_t* verdict, PhotoRec* rec) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n) return;
    const int c0 = it == 0 ? 0 : 2 + it, c1 = 2 + it;
    PhotoRec est = {0.0, 0.0, 0, 0};
    for (int c = c0; c <= c1; c++) {
        PhotoRec r = {0.0, 0.0, 0, 0};
#pragma unroll
        for (int s = 0; s < PHOTO_SLICES; s++) {
            const PhotoRec p = partial[((size_t)b * stride + c) * PHOTO_SLICES + s];
            r.sum += p.sum;
            r.sum_inside += p.sum_inside;
            r.n_inside += p.n_inside;
            r.flags |= p.flags;
        }
        if (c < c1) rec[(size_t)b * stride + c] = r;
        est = r;
    }
    const int id = ids[b];
    int v = it == 0 ? 0 : verdict[b];
    if (id >= 0 && id < n_sessions && gate[b] != 0 && updates[b] >= 0 && v == 0) {
        const PhotoGate g = gates[id];
        const PhotoRec pr = rec[(size_t)b * stride + 1];                       // (iteration 0 wrote it above, this lane)
        const hnet_ekf::PhotoRecord hp = {pr.sum, pr.sum_inside, pr.n_inside, pr.flags}, he = {est.sum, est.sum_inside, est.n_inside, est.flags};
        if (hnet_ekf::photo_reject(hp, he, g.max_ratio, g.min_inside)) {
            est.flags |= PHOTO_REJECTED;
            gate[b] = 0;
            v = 1 + it;
        }
    }
    rec[(size_t)b * stride + c1] = est;
    if (it == 0 || v == 1 + it) verdict[b] = v;
}

hipError_t photo_init_device() {
    hipError_t e = hipFuncSetAttribute((const void*)photo_iter_kernel<true, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, PH_ITER_LDS_STAGED);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)photo_iter_kernel<true, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, PH_ITER_LDS_STAGED);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void*)photo_residual_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PH_LDS_BYTES);
}

hipError_t launch_photo_iteration(const uint8_t* img1, const uint8_t* img2, int n, const PhotoCands& cands, int it, int iters, bool staged, PhotoRec* partial,
                                  const int32_t* ids, int n_sessions, const PhotoGate* gates, const int32_t* updates, int32_t* gate, int32_t* verdict, PhotoRec* rec,
                                  hipStream_t s) {
    if (n < 1 || n > (1 << 20) || it < 0 || it >= iters || 2 + iters > PHOTO_MAX_CAND || !img1 || !img2 || !partial || !rec) return hipErrorInvalidValue;
    if ((((uintptr_t)img1) & 3) || (((uintptr_t)img2) & 15) || cands.offsets || !cands.prior || !cands.net) return hipErrorInvalidValue;
    if (!ids || !gates || !updates || !gate || !verdict) return hipErrorInvalidValue;
    const int stride = 2 + iters;
    const dim3 grid((unsigned)(n * PHOTO_SLICES)), block(PH_THREADS);
    if (it == 0) hipLaunchKernelGGL((photo_iter_kernel<true, 3>), grid, block, PH_ITER_LDS_STAGED, s, img1, img2, cands, 0, stride, partial);      // (always staged)
    else if (staged) hipLaunchKernelGGL((photo_iter_kernel<true, 1>), grid, block, PH_ITER_LDS_STAGED, s, img1, img2, cands, 2 + it, stride, partial);
    else hipLaunchKernelGGL((photo_iter_kernel<false, 1>), grid, block, PH_ITER_LDS_GLOBAL, s, img1, img2, cands, 2 + it, stride, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(photo_gate_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, (const PhotoRec*)partial, n, it, stride, ids, n_sessions, gates, updates,
                       gate, verdict, rec);
    return hipGetLastError();
}

hipError_t launch_photo_residual(const uint8_t* img1, const uint8_t* img2, int n, const PhotoCands& cands, int m, PhotoRec* partial, PhotoRec* out, float* map,
                                 hipStream_t s) {
    if (n < 1 || n > (1 << 20) || m < 1 || m > PHOTO_MAX_CAND || !img1 || !img2 || !partial || !out) return hipErrorInvalidValue;
    if ((((uintptr_t)img1) & 3) || (((uintptr_t)img2 | (uintptr_t)map) & 15)) return hipErrorInvalidValue;
    if (!cands.offsets && ((m > 1 && !cands.prior) || (m > 2 && !cands.net))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(photo_residual_kernel, dim3((unsigned)(n * PHOTO_SLICES)), dim3(PH_THREADS), PH_LDS_BYTES, s, img1, img2, cands, m, partial, map);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int count = n * m;
    hipLaunchKernelGGL(photo_finish_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, s, (const PhotoRec*)partial, count, out);
    return hipGetLastError();
}

}  // namespace hnet
