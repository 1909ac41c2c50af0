// keyframe_render_ref.cpp — the host reference of rendering a keyframe map into a view (include/hnet.h hnet_op_keyframe_render,
// hnet_sessions_keyframe_render): render_setup, render_sample, render_pixel, seam_add and render_fit_view of include/hnet_keyframe_render.h,
// the very functions the device compiles, and one whole render on the host: image, cover and record.  Built as keyframe_map_ref.cpp is built (nothing
// may be contracted):
//   g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -D__HIP_PLATFORM_AMD__ -I <rocm>/include -I cuahn_vio_amd/csrc -I include tests/cpp/keyframe_render_ref.cpp
#include "geom.h"

#include <cmath>
#include <cstdint>
#include <cstring>

#include "hnet_keyframe_render.h"

namespace km = hnet_keyframe_map;
namespace kr = hnet_keyframe_render;

static_assert(sizeof(km::Entry) == 88 && sizeof(kr::Opts) == 16 && sizeof(kr::Record) == 224 && sizeof(kr::Counters) == 144,
              "the layouts of include/hnet.h and csrc/keyframe_render_dev.h");

extern "C" {

// 1 and S [9] written, or 0
int keyframe_render_ref_setup(const double* h_origin_view, const void* entry, double* S) {
    return kr::render_setup(h_origin_view, *static_cast<const km::Entry*>(entry), S) ? 1 : 0;
}

// 1 and *val written, or 0; img [224][320]
int keyframe_render_ref_sample(const double* S, const uint8_t* img, int u, int v, uint8_t* val) { return kr::render_sample(S, img, u, v, *val) ? 1 : 0; }

// one pixel from its samples vals [8] and their validity mask: the output byte; *cover written; with cover >= 2, n [8] and sse [8] advanced
int keyframe_render_ref_pixel(const uint8_t* vals, int mask, const int32_t* links, const int32_t* serial, int mode, int* cover, uint64_t* n, uint64_t* sse) {
    uint64_t packed = 0;
    for (int j = 0; j < kr::MAX_ENTRIES; j++) packed |= (uint64_t)vals[j] << (8 * j);
    const uint8_t out = kr::render_pixel(packed, mask, links, serial, mode, *cover);
    if (*cover >= 2) kr::seam_add(packed, mask, (int)out, n, sse);
    return out;
}

int keyframe_render_ref_fit_view(const void* entries, int capacity, int width, int height, double margin_px, double* h_origin_view) {
    return kr::render_fit_view(static_cast<const km::Entry*>(entries), capacity, width, height, margin_px, h_origin_view) ? 1 : 0;
}

int keyframe_render_ref_opts_valid(const void* opts) { return kr::opts_valid(*static_cast<const kr::Opts*>(opts)) ? 1 : 0; }

// the whole render of m entries with images [m][71 680] into the view: out_img and out_cover [height][width] and the record, every byte written
void keyframe_render_ref_render(int m, const uint8_t* images, const void* entries, const double* h_origin_view, const void* opts, uint8_t* out_img,
                                uint8_t* out_cover, void* rec) {
    const km::Entry* e = static_cast<const km::Entry*>(entries);
    const kr::Opts& o = *static_cast<const kr::Opts*>(opts);
    kr::Record& r = *static_cast<kr::Record*>(rec);
    double S[kr::MAX_ENTRIES * 9];
    int32_t links[kr::MAX_ENTRIES], serial[kr::MAX_ENTRIES];
    memset(&r, 0, sizeof r);
    memset(S, 0, sizeof S);
    for (int k = 0; k < 9; k++) r.h_origin_view[k] = h_origin_view[k];
    for (int j = 0; j < kr::MAX_ENTRIES; j++) links[j] = serial[j] = 0;
    for (int j = 0; j < m; j++) {
        if (kr::render_setup(h_origin_view, e[j], S + 9 * j)) {
            r.used_mask |= 1 << j;
            links[j] = e[j].links;
            serial[j] = e[j].serial;
        } else {
            r.skipped_mask |= 1 << j;
        }
    }
    for (int v = 0; v < o.height; v++)
        for (int u = 0; u < o.width; u++) {
            const size_t i = (size_t)v * o.width + u;
            out_img[i] = kr::render_one(S, r.used_mask, images, links, serial, m, o.mode, u, v, out_cover[i], r.c);
        }
}

}  // extern "C"
