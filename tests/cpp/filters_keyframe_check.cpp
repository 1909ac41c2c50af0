// filters_keyframe_check.cpp — the keyframe track as an in-step filter measurement (include/hnet_keyframe_measure.h) and the host reference around it
// (tests/cpp/filters_keyframe_ref.cpp) on fixed inputs, meant for AddressSanitizer + UBSan on the CPU:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I <rocm>/include
//       -I cuahn_vio_amd/csrc -I include tests/cpp/filters_keyframe_check.cpp -o filters_keyframe_check && ./filters_keyframe_check
// z on a pair of keys; each UNUSABLE reason on a synthetic record; six paths of hnet_ekf::iterated_update_keyframe_measured: the feature off, a first
// frame and the frame after it on heap frames of exactly 71 680 bytes through the host robust alignment (the second is applied), a measurement `when`
// keeps out, one the NIS gate refuses, and one applied from a stub record.
// Exit status 0 = all hold.
#include "filters_keyframe_ref.cpp"

#include <cstdio>
#include <cstdlib>

namespace {
int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

constexpr int CELL = 16, LW = 30, LH = 30, X0 = 72, Y0 = 120;

// a fixed smooth scene: bilinear interpolation of an LCG lattice (no library generator, so every platform sees the same bytes)
struct Scene {
    uint8_t lat[LH][LW];
    Scene() {
        uint32_t s = 2463534242u;
        for (int y = 0; y < LH; y++)
            for (int x = 0; x < LW; x++) {
                s = s * 1664525u + 1013904223u;
                lat[y][x] = (uint8_t)(s >> 24);
            }
    }
    uint8_t at(int x, int y) const {
        const int x0 = x / CELL, y0 = y / CELL, fx = x % CELL, fy = y % CELL;
        const int top = lat[y0][x0] * (CELL - fx) + lat[y0][x0 + 1] * fx, bot = lat[y0 + 1][x0] * (CELL - fx) + lat[y0 + 1][x0 + 1] * fx;
        return (uint8_t)((top * (CELL - fy) + bot * fy) / (CELL * CELL));
    }
    std::vector<uint8_t> view(int dx, int dy) const {
        std::vector<uint8_t> f(photo_ref::NPIX);
        for (int v = 0; v < photo_ref::IMG_H; v++)
            for (int u = 0; u < photo_ref::IMG_W; u++) f[v * photo_ref::IMG_W + u] = at(u + X0 - dx, v + Y0 - dy);
        return f;
    }
};

hnet_photo_robust record(int flags, double mse) {
    hnet_photo_robust r;
    memset(&r, 0, sizeof r);
    for (int k = 0; k < 8; k++) r.px.offsets_px[k] = 2.0f + 0.125f * (float)k;
    r.px.mse0 = 9.0; r.px.mse = mse; r.px.n_valid0 = r.px.n_valid = 70000; r.px.trials = 3; r.px.accepted = 2; r.px.flags = flags;
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 8; j++) r.px.info[i * 8 + j] = i == j ? 4000.0 + 100.0 * i : 50.0;
    return r;
}

hnet_keyframe_track track_of(const hnet_photo_robust& r, int flags) {
    hnet_keyframe_track t;
    memset(&t, 0, sizeof t);
    t.rec = r;
    t.flags = flags;
    return t;
}

hnet_filter_state filter_state(double off) {
    hnet_filter_state s;
    memset(&s, 0, sizeof s);
    s.t = 2.5;
    s.q[0] = 1.0;
    for (int c = 0; c < 4; c++) { s.offset[3 * c] = off * (c + 1); s.offset[3 * c + 1] = -off * (c + 2); }
    for (int i = 0; i < 27; i++) s.cov[i * 27 + i] = 1e-4;
    return s;
}

hnet_keyframe_measure_opts options(double cov_scale, int when) {
    hnet_keyframe_measure_opts o;
    filters_keyframe_ref_default_opts(&o);
    o.track.levels = 2;
    o.track.align.base.max_iterations = 3;
    o.cov_scale = cov_scale;
    o.when = when;
    return o;
}

struct Loop {
    hnet_filter_state st;
    std::vector<hnet_innovation> out;
    std::vector<hnet_photo_residual> prec;
    hnet_keyframe_measure rec;
    int updates, calls, align_calls, copy;
};

Loop run(const hnet_filter_state& st0, const hnet_filter_params& p, const std::vector<float>& net, int iters, int gate, double max_nis, const hnet_keyframe_measure_opts* m,
         kfm::Session& ks, uint8_t* keyframe, const uint8_t* curr, const hnet_photo_robust* stub, int accepted) {
    Loop l;
    l.st = st0;
    l.out.resize(iters);
    l.prec.resize(1 + iters);
    std::vector<hnet_photo_residual> script(1 + iters);
    memset(script.data(), 0, script.size() * sizeof(hnet_photo_residual));
    l.updates = filters_keyframe_ref_iterated(&l.st, &p, iters, net.data(), gate, max_nis, script.data(), 0.0, 0, m, 0, &ks, keyframe, curr, stub, accepted, l.out.data(),
                                              l.prec.data(), &l.rec, &l.calls, &l.align_calls, nullptr, &l.copy);
    return l;
}
}  // namespace

int main() {
    // z: equal keys give zeros, a zero previous key the current one, a key without a homography nothing
    float kp[8], kc[8], z[8];
    for (int k = 0; k < 8; k++) { kp[k] = 1.5f - 0.5f * (float)k; kc[k] = 3.0f + 0.25f * (float)k; }
    const float zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    CHECK(filters_keyframe_ref_relative_z(kp, kp, z) == 1);
    for (int k = 0; k < 8; k++) CHECK(std::fabs(z[k]) < 1e-5f);
    CHECK(filters_keyframe_ref_relative_z(zero, kc, z) == 1 && memcmp(z, kc, sizeof z) == 0);
    float line[8];
    for (int c = 0; c < 4; c++) { line[2 * c] = (float)(10.0 * c - hnet::p4(2 * c)); line[2 * c + 1] = (float)(5.0 * c - hnet::p4(2 * c + 1)); }
    CHECK(filters_keyframe_ref_relative_z(line, kc, z) == 0);

    // the eleven reasons, each alone
    const hnet_photo_robust good = record(0, 4.0);
    hnet_keyframe_measure_opts o = options(1.0, HNET_KFM_ALWAYS);
    double r_px[64];
    float out72[72];
    int32_t fl = 0;
    hnet_keyframe_track t = track_of(good, 0);
    CHECK(filters_keyframe_ref_measure(1, kp, 1, &t, 2, &o, 10.0, z, r_px, out72, &fl) == 1 && fl == 0);
    struct Case { int had_key; const float* key; int prev_ok; hnet_keyframe_track t; int accepted; hnet_keyframe_measure_opts o; double k; int bit; };
    hnet_photo_robust stopped = record(hnet_align::SINGULAR, 4.0), flat = good, huge = record(0, 1e308);
    memset(flat.px.info, 0, sizeof flat.px.info);
    hnet_keyframe_measure_opts mse_o = o, big_o = o;
    mse_o.max_mse = 3.0;
    big_o.cov_scale = 1e10;
    const Case cases[11] = {
        {0, kp, 1, track_of(good, 0), 2, o, 10.0, HNET_KFM_FIRST},
        {1, kp, 1, track_of(good, HNET_KF_STOPPED | HNET_KF_REKEYED), 2, o, 10.0, HNET_KFM_TRACK_LOST},
        {1, kp, 1, track_of(good, HNET_KF_GAP), 2, o, 10.0, HNET_KFM_TRACK_GAP},
        {1, kp, 0, track_of(good, 0), 2, o, 10.0, HNET_KFM_PREV_NOT_MEASURED},
        {1, line, 1, track_of(good, 0), 2, o, 10.0, HNET_KFM_NO_INVERSE},
        {1, kp, 1, track_of(good, 0), 2, o, 0.0, HNET_KFM_BAD_K_NET_COV},
        {1, kp, 1, track_of(stopped, 0), 2, o, 10.0, HNET_KFM_STOPPED},
        {1, kp, 1, track_of(good, 0), 0, o, 10.0, HNET_KFM_NO_STEP},
        {1, kp, 1, track_of(good, 0), 2, mse_o, 10.0, HNET_KFM_MSE_ABOVE_MAX},
        {1, kp, 1, track_of(flat, 0), 2, o, 10.0, HNET_KFM_NO_FACTOR},
        {1, kp, 1, track_of(huge, 0), 2, big_o, 10.0, HNET_KFM_NON_FINITE},
    };
    for (const Case& c : cases) {
        fl = 0;
        CHECK(filters_keyframe_ref_measure(c.had_key, c.key, c.prev_ok, &c.t, c.accepted, &c.o, c.k, z, r_px, out72, &fl) == 0 && fl == c.bit);
    }

    // the loop
    hnet_filter_params p;
    memset(&p, 0, sizeof p);
    p.k_net_cov = 10.0;
    const int iters = 2;
    const hnet_filter_state st = filter_state(3.0 / 159.5 / 4.0);
    std::vector<float> net((size_t)iters * 72, 0.0f);
    for (int it = 0; it < iters; it++)
        for (int i = 0; i < 8; i++) {
            net[it * 72 + i] = (float)(st.offset[3 * (i >> 1) + (i & 1)] * 159.5) + 0.1f * (float)(i - 3);
            net[it * 72 + 8 + i * 9] = 2.0f;
        }
    kfm::Session none;
    memset(&none, 0, sizeof none);
    // 1 the feature off: the record is zero, the aligner idle
    kfm::Session ks = none;
    Loop l = run(st, p, net, iters, 1, 0.0, nullptr, ks, nullptr, nullptr, &good, 2);
    hnet_keyframe_measure zero_rec;
    memset(&zero_rec, 0, sizeof zero_rec);
    CHECK(l.updates == iters && l.align_calls == 0 && memcmp(&l.rec, &zero_rec, sizeof zero_rec) == 0 && memcmp(&ks, &none, sizeof ks) == 0);
    // 2, 3 heap frames through the host robust alignment: a first frame, then the view (3, 2) px on with a state whose offsets say about that
    const Scene scene;
    std::vector<uint8_t> key(photo_ref::NPIX, 0), f0 = scene.view(0, 0), f1 = scene.view(3, 2);
    hnet_keyframe_measure_opts oi = options(1.0, HNET_KFM_IF_NONE);
    Loop a = run(st, p, net, iters, 0, 0.0, &oi, ks, key.data(), f0.data(), nullptr, 0);
    CHECK(a.rec.flags == (HNET_KFM_ASKED | HNET_KFM_FIRST) && a.copy == 1 && a.align_calls == 0 && a.updates == 0 && memcmp(key.data(), f0.data(), photo_ref::NPIX) == 0);
    CHECK(ks.key.has_key == 1 && ks.prev_ok == 1 && (a.rec.track.flags & HNET_KF_FIRST));
    hnet_filter_state moving = filter_state(0.0);
    for (int c = 0; c < 4; c++) { moving.offset[3 * c] = 2.8 / 159.5; moving.offset[3 * c + 1] = 2.1 / 159.5; }
    Loop b = run(moving, p, net, iters, 0, 0.0, &oi, ks, key.data(), f1.data(), nullptr, 0);
    CHECK(b.align_calls == 1 && b.rec.flags == (HNET_KFM_ASKED | HNET_KFM_APPLIED) && b.updates == 1 && b.rec.innov.flag == HNET_INNOV_USED);
    for (int c = 0; c < 4; c++) CHECK(std::fabs(b.rec.z_px[2 * c] - 3.0f) < 0.25f && std::fabs(b.rec.z_px[2 * c + 1] - 2.0f) < 0.25f);
    CHECK(ks.prev_ok == 1 && ks.key.age == 1);
    // 4 .. 6 a stub record near compose(step, key_px): IF_NONE after applied updates, a refused NIS, and applied
    kfm::Session held = none;
    held.key.has_key = 1; held.key.keyframes = 1; held.prev_ok = 1;
    for (int k = 0; k < 9; k++) held.key.h_origin_key[k] = (k & 3) == 0 ? 1.0 : 0.0;
    hnet_photo_robust near = good;
    for (int k = 0; k < 8; k++) near.px.offsets_px[k] = (float)(st.offset[3 * (k >> 1) + (k & 1)] * 159.5) + 0.05f * (float)k;
    ks = held;
    Loop c4 = run(st, p, net, iters, 1, 0.0, &oi, ks, nullptr, nullptr, &near, 2);
    CHECK(c4.rec.flags == (HNET_KFM_ASKED | HNET_KFM_NOT_SELECTED) && c4.updates == iters && c4.align_calls == 1);
    ks = held;
    Loop c5 = run(st, p, net, iters, 0, 1e-30, &o, ks, nullptr, nullptr, &near, 2);
    CHECK(c5.rec.flags == (HNET_KFM_ASKED | HNET_KFM_NIS_REJECTED) && c5.updates == 0 && c5.rec.innov.flag == HNET_INNOV_REJECTED);
    ks = held;
    Loop c6 = run(st, p, net, iters, 1, 0.0, &o, ks, nullptr, nullptr, &near, 2);
    CHECK(c6.rec.flags == (HNET_KFM_ASKED | HNET_KFM_APPLIED) && c6.updates == iters + 1 && c6.rec.innov.iteration == iters && ks.key.age == 1);
    for (int c = 0; c < 4; c++)
        for (int k = 0; k < 3; k++) CHECK(c6.st.offset[3 * c + k] == 0.0);
    if (failures) {
        printf("filters keyframe check: %d FAILED\n", failures);
        return 1;
    }
    printf("filters keyframe check: z, 11 unusable cases, 6 loop paths (2 applied) ok\n");
    return 0;
}
