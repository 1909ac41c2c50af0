// kernels_keyframe_render.hip — the device side of rendering a keyframe map into a view (include/hnet.h hnet_op_keyframe_render,
// hnet_sessions_keyframe_render).  Two launches: the setup, one wavefront per slot, fp64 in registers, composes for each of the M entries
// where a pixel of the view samples it (include/hnet_keyframe_render.h render_setup) and zeroes the slot's record; the render gathers, blends and counts.
// Like kernels_keyframe_map.hip built with -ffp-contract=off: every function is the host reference's in its order.
//
// The render's tile is 64 x 16 pixels per workgroup of 256 lanes: one pixel per lane and step, four steps, and in every step a wavefront holds ONE row
// of 64 consecutive pixels.  So the two stores of a step (image, cover) are 64 consecutive bytes per wavefront, and under a view close to the keyframes'
// own scale and orientation - what a map of one flight is - the taps of a wavefront fall into one or two rows of a stored image, a few cache lines per
// gather.  16 rows bound what a tile touches of one image under a rotated view and keep the partial tiles of the bottom edge cheap; the eight images of
// a session (573 KB) stay in L2 either way, so nothing is staged in LDS: the taps are direct u8 gathers.  The slot's table (648 bytes) is uniform over the
// workgroup and is read with scalar loads through the scalar cache: staged in LDS, its 144 words were hoisted into vector registers (226 of them, two
// waves per SIMD); as scalars the kernel holds 66 and seven waves per SIMD hide the gathers.  The 2 + 2 M counters are summed per lane in 32 bits (a
// workgroup adds at most 1024 x 255^2), reduced by shuffles over the wavefront and through LDS over the workgroup, and added to the slot's record with
// one 64-bit atomic add per non-zero counter: integers, so the order of the workgroups does not show in the bits (7g's rule).  Nothing waits on another
// workgroup.  The host side is capi_keyframe_render.hip.
#include "keyframe_render_dev.h"

namespace hnet {

namespace km = hnet_keyframe_map;
namespace kr = hnet_keyframe_render;

namespace {
constexpr int N_COUNTERS = 2 + 2 * RENDER_MAX;
static_assert(sizeof(kr::Counters) == N_COUNTERS * sizeof(uint64_t), "the record's counters, as 64-bit words");
static_assert(RENDER_TILE_W == 64 && RENDER_TILE_H % 4 == 0, "a row of the tile per wavefront and step, four wavefronts");
static_assert(kr::KEY_PIXELS == NPIX, "the stored keyframes are frames");

__device__ inline bool source_ok(const RenderSource& src) { return src.capacity >= 1 && src.capacity <= RENDER_MAX; }
__device__ inline uint32_t wave_sum(uint32_t x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}
}  // namespace

__global__ __launch_bounds__(KEY_THREADS) void keyframe_render_setup_kernel(const int32_t* __restrict__ ids, int n, RenderSource src, const double* __restrict__ views,
                                                                            RenderTab* __restrict__ tab, RenderRec* __restrict__ rec) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= n) return;
    const int id = ids[b];
    const bool valid = id >= 0 && id < src.n_sessions && source_ok(src);                 // (uniform over the wavefront)
    double hv[9];
    for (int k = 0; k < 9; k++) hv[k] = (k & 3) == 0 ? 1.0 : 0.0;
    if (views) {
        for (int k = 0; k < 9; k++) hv[k] = views[(size_t)b * 9 + k];
    } else if (valid && src.state) {
        const KeyState s = src.state[id];
        if (s.has_key) (void)km::origin_curr(s, hv);                                       // (false: the state's h_origin_key, which the setups then judge)
    }
    const bool mine = valid && t < src.capacity;
    bool ok = false;
    double S[9];
    for (int k = 0; k < 9; k++) S[k] = 0.0;
    int32_t links = 0, serial = 0;
    if (mine) {
        const MapEntry e = src.entry[(size_t)id * src.capacity + t];
        ok = kr::render_setup(hv, e, S);
        links = e.links;
        serial = e.serial;
    }
    const int used = (int)(__ballot(ok) & 0xffu), tried = (int)(__ballot(mine) & 0xffu);
    if (t < RENDER_MAX) {
        for (int k = 0; k < 9; k++) tab[b].S[t][k] = ok ? S[k] : 0.0;
        tab[b].links[t] = ok ? links : 0;
        tab[b].serial[t] = ok ? serial : 0;
    }
    uint64_t* cnt = reinterpret_cast<uint64_t*>(&rec[b].c);
    if (t < N_COUNTERS) cnt[t] = 0;
    if (t != 0) return;
    tab[b].used_mask = used;
    tab[b].pad = 0;
    for (int k = 0; k < 9; k++) rec[b].h_origin_view[k] = hv[k];
    rec[b].used_mask = used;
    rec[b].skipped_mask = tried & ~used;
}

__global__ __launch_bounds__(256) void keyframe_render_kernel(const int32_t* __restrict__ ids, RenderSource src, const RenderTab* __restrict__ tab, int width,
                                                              int height, int mode, int tiles_x, uint8_t* __restrict__ out_img, uint8_t* __restrict__ out_cover,
                                                              RenderRec* rec) {
    __shared__ uint32_t part[4][N_COUNTERS];
    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const RenderTab& st = tab[b];                                                          // (uniform: scalar loads, the table never occupies vector registers)
    const int id = ids[b];
    const bool valid = id >= 0 && id < src.n_sessions && source_ok(src);
    const int ok_mask = valid ? st.used_mask & ((1 << src.capacity) - 1) : 0;              // (no bit: no image of the source is addressed)
    const uint8_t* img = src.img + (valid ? (size_t)id * src.capacity * NPIX : 0);
    const int u = (int)(blockIdx.x % (unsigned)tiles_x) * RENDER_TILE_W + lane, v0 = (int)(blockIdx.x / (unsigned)tiles_x) * RENDER_TILE_H + wave;
    uint32_t cnt[N_COUNTERS];
#pragma unroll
    for (int k = 0; k < N_COUNTERS; k++) cnt[k] = 0;
    for (int step = 0; step < RENDER_TILE_H / 4; step++) {
        const int v = v0 + 4 * step;
        if (u >= width || v >= height) continue;                                           // (the partial tiles of the right and the bottom edge)
        uint64_t vals = 0;
        int mask = 0, cover = 0;
#pragma unroll
        for (int j = 0; j < RENDER_MAX; j++) {
            uint8_t val = 0;
            if (!((ok_mask >> j) & 1) || !kr::render_sample(st.S[j], img + (size_t)j * NPIX, u, v, val)) continue;
            vals |= (uint64_t)val << (8 * j);
            mask |= 1 << j;
        }
        const uint8_t out = kr::render_pixel(vals, mask, st.links, st.serial, mode, cover);
        const size_t o = ((size_t)b * height + v) * width + u;
        out_img[o] = out;
        out_cover[o] = (uint8_t)cover;
        if (cover >= 1) cnt[0]++;
        if (cover >= 2) {
            cnt[1]++;
            kr::seam_add(vals, mask, (int)out, cnt + 2, cnt + 2 + RENDER_MAX);
        }
    }
#pragma unroll
    for (int k = 0; k < N_COUNTERS; k++) {
        const uint32_t w = wave_sum(cnt[k]);
        if (lane == 0) part[wave][k] = w;
    }
    __syncthreads();
    if (t >= N_COUNTERS) return;
    const uint32_t sum = (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
    if (sum != 0) atomicAdd(reinterpret_cast<unsigned long long*>(&rec[b].c) + t, (unsigned long long)sum);
}

hipError_t launch_keyframe_render_setup(const int32_t* ids, int n, const RenderSource& src, const double* views, RenderTab* tab, RenderRec* rec, hipStream_t s) {
    if (n < 1 || n > 65535 || !ids || !tab || !rec || src.capacity < 1 || src.capacity > RENDER_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyframe_render_setup_kernel, dim3((unsigned)n), dim3(KEY_THREADS), 0, s, ids, n, src, views, tab, rec);
    return hipGetLastError();
}

hipError_t launch_keyframe_render(const int32_t* ids, int n, const RenderSource& src, const RenderTab* tab, const RenderOpts& opts, uint8_t* out_img,
                                  uint8_t* out_cover, RenderRec* rec, hipStream_t s) {
    if (n < 1 || n > 65535 || !ids || !tab || !rec || !out_img || !out_cover || !kr::opts_valid(opts) || src.capacity < 1 || src.capacity > RENDER_MAX)
        return hipErrorInvalidValue;
    const int tiles_x = (opts.width + RENDER_TILE_W - 1) / RENDER_TILE_W, tiles_y = (opts.height + RENDER_TILE_H - 1) / RENDER_TILE_H;
    hipLaunchKernelGGL(keyframe_render_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)n), dim3(256), 0, s, ids, src, tab, opts.width, opts.height, opts.mode,
                       tiles_x, out_img, out_cover, rec);
    return hipGetLastError();
}

}  // namespace hnet
