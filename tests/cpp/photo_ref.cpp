// photo_ref.cpp — the host reference of the photometric residual records (include/hnet.h hnet_photo_residual): the sampler of csrc/warp_dev.h restated in
// host fp32 (fmaf from <cmath>, IEEE division) on csrc/geom.h's dlt_solve, summed in double in ascending pixel order.
// Build (the sampler's roundings are written out, so nothing may be contracted behind its back):
//   g++ -std=c++17 -O2 -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I <rocm>/include -I cuahn_vio_amd/csrc -DPHOTO_REF_MAIN tests/cpp/photo_ref.cpp -o photo_ref
// The program reads {int32 n, int32 m, img1 u8 [n][224][320], img2 u8 [n][224][320], offsets f32 [n][m][8]} from the file named on its command line and prints
// one line per (pair, candidate): pair candidate sum sum_inside n_inside flags n_edge  (doubles with 17 digits).
// Without -DPHOTO_REF_MAIN (and with -shared -fPIC) it is a library with the same core behind photo_ref_records (tests, tools).
#include "geom.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace photo_ref {

using hnet::IMG_H;
using hnet::IMG_W;
using hnet::NPIX;

struct Record { double sum, sum_inside; int32_t n_inside, flags; };
constexpr int DEGENERATE = 1;

// H = (float) dlt_solve(p4 + offsets), the corners an fp32 sum; a non-finite entry makes the matrix all NaN (returns false)
inline bool homography(const float* off, float* h) {
    double d[8], hd[9];
    for (int k = 0; k < 8; k++) d[k] = (double)(float)(hnet::p4(k) + (double)off[k]);
    hnet::dlt_solve(d, hd);
    bool ok = true;
    for (int k = 0; k < 9; k++) ok = ok && std::isfinite((float)hd[k]);
    for (int k = 0; k < 9; k++) h[k] = ok ? (float)hd[k] : NAN;
    return ok;
}

// warp_coords (csrc/warp_dev.h): the quotients are IEEE divisions there too (its reciprocal form is bit-identical to x / z); the device build contracts
// q * (2 / (W - 1)) - 1 into one FMA
inline void coords(const float* h, int u, int v, float& ix, float& iy) {
    const float fu = (float)u, fv = (float)v;
    const float X = fmaf(h[0], fu, fmaf(h[1], fv, h[2]));
    const float Y = fmaf(h[3], fu, fmaf(h[4], fv, h[5]));
    const float Z = fmaf(h[6], fu, fmaf(h[7], fv, h[8]));
    const float qx = X / Z, qy = Y / Z;
    const float gx = fmaf(qx, (float)(2.0 / (IMG_W - 1)), -1.0f);
    const float gy = fmaf(qy, (float)(2.0 / (IMG_H - 1)), -1.0f);
    ix = ((gx + 1.0f) * 0.5f) * (float)(IMG_W - 1);
    iy = ((gy + 1.0f) * 0.5f) * (float)(IMG_H - 1);
}

inline float unit(uint8_t b) { return (float)b / 255.0f; }

// warp_taps_global (csrc/warp_dev.h): the four-tap blend, taps outside the image contribute 0, NaN / far-out positions give 0
inline float taps(const uint8_t* img, float ix, float iy) {
    const float x0f = floorf(ix), y0f = floorf(iy);
    if (!(x0f >= -1.0f && x0f <= (float)IMG_W && y0f >= -1.0f && y0f <= (float)IMG_H)) return 0.0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const float wx1 = ix - x0f, wx0 = 1.0f - wx1, wy1 = iy - y0f, wy0 = 1.0f - wy1;
    const bool xin0 = x0 >= 0 && x0 < IMG_W, xin1 = x0 + 1 >= 0 && x0 + 1 < IMG_W;
    const bool yin0 = y0 >= 0 && y0 < IMG_H, yin1 = y0 + 1 >= 0 && y0 + 1 < IMG_H;
    float s = 0.0f;
    if (yin0 && xin0) s = fmaf(unit(img[y0 * IMG_W + x0]), wx0 * wy0, s);
    if (yin0 && xin1) s = fmaf(unit(img[y0 * IMG_W + x0 + 1]), wx1 * wy0, s);
    if (yin1 && xin0) s = fmaf(unit(img[(y0 + 1) * IMG_W + x0]), wx0 * wy1, s);
    if (yin1 && xin1) s = fmaf(unit(img[(y0 + 1) * IMG_W + x0 + 1]), wx1 * wy1, s);
    return s;
}

inline bool near_bound(float x, float hi) { return fabsf(x + 0.5f) < 1e-3f || fabsf(x - hi) < 1e-3f; }

// one record; n_edge (may be null): pixels whose ix or iy lies within 1e-3 px of one of the four inside bounds; map (may be null): e per pixel [NPIX]
inline Record record(const uint8_t* img1, const uint8_t* img2, const float* off, int32_t* n_edge, float* map) {
    float h[9];
    Record r = {0.0, 0.0, 0, homography(off, h) ? 0 : DEGENERATE};
    int32_t edge = 0;
    for (int v = 0; v < IMG_H; v++)
        for (int u = 0; u < IMG_W; u++) {
            float ix, iy;
            coords(h, u, v, ix, iy);
            const float e = fabsf(taps(img2, ix, iy) - unit(img1[v * IMG_W + u])) * 255.0f;
            const bool in = -0.5f < ix && ix < (float)IMG_W - 0.5f && -0.5f < iy && iy < (float)IMG_H - 0.5f;
            r.sum += (double)e;
            if (in) { r.sum_inside += (double)e; r.n_inside++; }
            if (near_bound(ix, (float)IMG_W - 0.5f) || near_bound(iy, (float)IMG_H - 0.5f)) edge++;
            if (map) map[v * IMG_W + u] = e;
        }
    if (n_edge) *n_edge = edge;
    return r;
}

}  // namespace photo_ref

extern "C" {

// records [n][m] (24 bytes each: sum, sum_inside, n_inside, flags), n_edge [n][m] or null, map [n][m][NPIX] or null
void photo_ref_records(const uint8_t* img1, const uint8_t* img2, int n, const float* offsets, int m, void* out, int32_t* n_edge, float* map) {
    static_assert(sizeof(photo_ref::Record) == 24, "the record layout of hnet_photo_residual");
    photo_ref::Record* o = static_cast<photo_ref::Record*>(out);
    for (int b = 0; b < n; b++)
        for (int c = 0; c < m; c++) {
            const size_t i = (size_t)b * m + c;
            o[i] = photo_ref::record(img1 + (size_t)b * photo_ref::NPIX, img2 + (size_t)b * photo_ref::NPIX, offsets + i * 8, n_edge ? n_edge + i : nullptr,
                                     map ? map + i * photo_ref::NPIX : nullptr);
        }
}

// H [n][9] = photo_ref::homography of offsets [n][8] (all NaN where ok [n] is 0): what the device's matrices are held against bit for bit
void photo_ref_homography(int n, const float* offsets, float* H, int32_t* ok) {
    for (int b = 0; b < n; b++) ok[b] = photo_ref::homography(offsets + b * 8, H + b * 9) ? 1 : 0;
}

}  // extern "C"

#ifdef PHOTO_REF_MAIN
int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s input.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t hdr[2];
    if (fread(hdr, sizeof hdr, 1, f) != 1 || hdr[0] < 1 || hdr[0] > 4096 || hdr[1] < 1 || hdr[1] > 66) { fprintf(stderr, "bad header\n"); fclose(f); return 2; }
    const int n = hdr[0], m = hdr[1];
    std::vector<uint8_t> i1((size_t)n * photo_ref::NPIX), i2(i1.size());
    std::vector<float> off((size_t)n * m * 8);
    const bool ok = fread(i1.data(), 1, i1.size(), f) == i1.size() && fread(i2.data(), 1, i2.size(), f) == i2.size() &&
                    fread(off.data(), sizeof(float), off.size(), f) == off.size();
    fclose(f);
    if (!ok) { fprintf(stderr, "short input\n"); return 2; }
    std::vector<photo_ref::Record> rec((size_t)n * m);
    std::vector<int32_t> edge(rec.size());
    photo_ref_records(i1.data(), i2.data(), n, off.data(), m, rec.data(), edge.data(), nullptr);
    for (int b = 0; b < n; b++)
        for (int c = 0; c < m; c++) {
            const photo_ref::Record& r = rec[(size_t)b * m + c];
            printf("%d %d %.17g %.17g %d %d %d\n", b, c, r.sum, r.sum_inside, r.n_inside, r.flags, edge[(size_t)b * m + c]);
        }
    return 0;
}
#endif
