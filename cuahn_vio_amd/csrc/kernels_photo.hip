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
#include "photo_dev.h"
#include "warp_dev.h"

namespace hnet {

namespace {
constexpr int PH_THREADS = 256, PH_WAVES = PH_THREADS / 64;
constexpr int PH_QUADS = PHOTO_SLICE_PIX / (4 * PH_THREADS);                  // 10 quads per thread and candidate
// dynamic LDS: img2 | H [66][9] f32 | flags [66] i32 | per-wave sums [66][4] f64 x 2 | per-wave counts [66][4] i32
constexpr int PH_OFF_H = NPIX;
constexpr int PH_OFF_FLAG = PH_OFF_H + PHOTO_MAX_CAND * 9 * 4;
constexpr int PH_OFF_SUM = PH_OFF_FLAG + PHOTO_MAX_CAND * 4;
constexpr int PH_OFF_SIN = PH_OFF_SUM + PHOTO_MAX_CAND * PH_WAVES * 8;
constexpr int PH_OFF_CNT = PH_OFF_SIN + PHOTO_MAX_CAND * PH_WAVES * 8;
constexpr int PH_LDS_BYTES = PH_OFF_CNT + PHOTO_MAX_CAND * PH_WAVES * 4;      // 79 600: two workgroups per CU
static_assert(PH_OFF_H % 16 == 0 && PH_OFF_SUM % 8 == 0, "LDS sections aligned for their types");
static_assert(2 * PH_LDS_BYTES <= 160 * 1024, "two workgroups share a CU's LDS");

// one fixed tree over the 64 lanes; the total ends in lane 0
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    return v;
}
}  // namespace

// grid: PHOTO_SLICES * n workgroups (slice = block % PHOTO_SLICES); partial [n][m][PHOTO_SLICES]
__global__ __launch_bounds__(PH_THREADS) void photo_residual_kernel(const uint8_t* __restrict__ img1, const uint8_t* __restrict__ img2, PhotoCands cands, int m,
                                                                    PhotoRec* __restrict__ partial, float* __restrict__ map) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ph_lds[];
    uint8_t* tile = ph_lds;
    float* hs = reinterpret_cast<float*>(ph_lds + PH_OFF_H);
    int* fl = reinterpret_cast<int*>(ph_lds + PH_OFF_FLAG);
    double* w_sum = reinterpret_cast<double*>(ph_lds + PH_OFF_SUM);
    double* w_sin = reinterpret_cast<double*>(ph_lds + PH_OFF_SIN);
    int* w_cnt = reinterpret_cast<int*>(ph_lds + PH_OFF_CNT);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pair = blockIdx.x / PHOTO_SLICES, slice = blockIdx.x - pair * PHOTO_SLICES;

    // img2 of the pair -> LDS, 16 bytes per lane
    const uint4* src = reinterpret_cast<const uint4*>(img2 + (size_t)pair * NPIX);
    for (int i = tid; i < NPIX / 16; i += PH_THREADS) reinterpret_cast<uint4*>(tile)[i] = src[i];
    // the m matrices: H = (float) dlt_solve(p4 + offsets), the corners an fp32 sum as in dlt_kernel; a non-finite entry makes the whole matrix NaN, so that
    // every sampling position is NaN: every sample 0, no pixel inside
    if (tid < m) {
        const float* o = nullptr;
        if (cands.offsets) o = cands.offsets + ((size_t)pair * m + tid) * 8;
        else if (tid == 1) o = cands.prior + (size_t)pair * 8;
        else if (tid >= 2) o = cands.net + (size_t)(tid - 2) * cands.net_iter_stride + (size_t)pair * 72;
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
        float* mp = map ? map + ((size_t)pair * m + c) * NPIX : nullptr;
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
        partial[((size_t)pair * m + tid) * PHOTO_SLICES + slice] = r;
    }
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

hipError_t photo_init_device() {
    return hipFuncSetAttribute((const void*)photo_residual_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PH_LDS_BYTES);
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
