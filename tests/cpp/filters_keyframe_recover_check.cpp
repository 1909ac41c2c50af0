// filters_keyframe_recover_check.cpp — recovering a lost camera inside the in-step keyframe track (include/hnet_keyframe_measure_recover.h) and the host
// reference around it (tests/cpp/filters_keyframe_recover_ref.cpp) on fixed inputs, meant for AddressSanitizer + UBSan on the CPU:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I <rocm>/include
//       -I cuahn_vio_amd/csrc -I include tests/cpp/filters_keyframe_recover_check.cpp -o filters_keyframe_recover_check && ./filters_keyframe_recover_check
// The rule on heap records of exact size: the order of the reasons, the next prev_ok, measure_recover off against hnet_kfm::measure and on a RETRACKED
// and an ATTACHED record.  Then one row through hnet_ekf::iterated_update_keyframe_recovered on heap frames of exactly 71 680 bytes, without a map and
// with one of 3 slots: a first frame, an honest frame, with the map a constant frame (lost and unrecovered), a frame (64, -48) px away (recovered on
// the held keyframe: FROM_RELOC and applied; with the map: REATTACHED), and the next frame with the true step (applied).
// Exit status 0 = all hold.
#include "filters_keyframe_recover_ref.cpp"

#include <cstdio>
#include <cstdlib>
#include <memory>

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

// a usable level-0 record on the heap, exactly its size
std::unique_ptr<hnet_robust::Record> record(float first, double mse, int flags) {
    std::unique_ptr<hnet_robust::Record> r(new hnet_robust::Record);
    memset(r.get(), 0, sizeof *r);
    for (int k = 0; k < 8; k++) r->px.offsets_px[k] = first + 0.125f * (float)k;
    r->px.mse0 = 9.0; r->px.mse = mse; r->px.n_valid0 = r->px.n_valid = 70000; r->px.trials = 3; r->px.accepted = 2; r->px.flags = flags;
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 8; j++) r->px.info[i * 8 + j] = i == j ? 4000.0 + 100.0 * i : 50.0;
    return r;
}

void rule() {
    CHECK(kfmr::usable_recover(false, kf::STOPPED | kr::RECOVERED, rl::RL_ATTACHED, 0) == kfm::FIRST);
    CHECK(kfmr::usable_recover(true, kf::STOPPED | kf::GAP, rl::RL_ATTACHED, 0) == kfm::TRACK_LOST);
    CHECK(kfmr::usable_recover(true, kf::STOPPED | kr::RECOVERED | kf::GAP, rl::RL_ATTACHED, 0) == kfmr::REATTACHED);
    CHECK(kfmr::usable_recover(true, kf::STOPPED | kr::RECOVERED | kf::GAP, rl::RL_RETRACKED, 0) == kfm::TRACK_GAP);
    CHECK(kfmr::usable_recover(true, kf::STOPPED | kr::RECOVERED, rl::RL_RETRACKED, 0) == kfm::PREV_NOT_MEASURED);
    CHECK(kfmr::usable_recover(true, kf::STOPPED | kr::RECOVERED, rl::RL_RETRACKED, 1) == 0 && kfmr::usable_recover(true, 0, 0, 1) == 0);
    for (int bit : {(int)kf::NO_START, (int)kf::STOPPED, (int)kf::MSE_ABOVE_MAX, (int)kf::NON_FINITE}) {
        CHECK(kfmr::next_prev_ok_recover(bit | kf::BRIDGED) == 0 && kfmr::next_prev_ok_recover(bit | kf::BRIDGED | kr::RECOVERED) == 1);
        CHECK(kfm::next_prev_ok(bit) == 0);
    }
    CHECK(kfmr::next_prev_ok_recover(0) == 1 && kfmr::next_prev_ok_recover(kf::FIRST | kf::REKEYED) == 1);
    CHECK((kfmr::UNUSABLE & ~kfm::UNUSABLE) == kfmr::REATTACHED && !(kfmr::UNUSABLE & kfmr::FROM_RELOC));

    // heap records of exact size: a read or write past either shows
    const auto good = record(2.0f, 4.0, 0), other = record(5.0f, 6.0, 0), bad = record(2.0f, 900.0, hnet_align::DEGENERATE);
    std::unique_ptr<kf::Track> tr(new kf::Track), lost(new kf::Track);
    std::unique_ptr<kr::Reloc> zero(new kr::Reloc), re(new kr::Reloc);
    memset(tr.get(), 0, sizeof *tr);
    memset(lost.get(), 0, sizeof *lost);
    memset(re.get(), 0, sizeof *re);
    kr::zero_reloc(*zero);
    tr->rec = *good;
    lost->rec = *bad;
    lost->flags = kf::STOPPED | kf::BRIDGED | kr::RECOVERED;
    re->rv.rec = *other;
    kfm::Opts o;
    kfm::default_opts(o);
    o.cov_scale = 2.0;
    const float key_prev[8] = {1.0f, -0.5f, 0.75f, 0.25f, -1.0f, 0.5f, 0.125f, -0.25f};
    std::unique_ptr<float[]> z(new float[8]), z2(new float[8]), m72(new float[72]), m72b(new float[72]);
    std::unique_ptr<double[]> r_px(new double[64]), r_px2(new double[64]);
    int32_t fl = 0, fl2 = 0;
    // off: hnet_kfm::measure, bit for bit
    CHECK(kfmr::measure_recover(true, key_prev, 1, *tr, 2, *zero, 0, o, 10.0, z.get(), r_px.get(), m72.get(), fl));
    CHECK(kfm::measure(true, key_prev, 1, *tr, 2, o, 10.0, z2.get(), r_px2.get(), m72b.get(), fl2));
    CHECK(fl == 0 && fl2 == 0 && memcmp(z.get(), z2.get(), 32) == 0 && memcmp(r_px.get(), r_px2.get(), 512) == 0 && memcmp(m72.get(), m72b.get(), 288) == 0);
    // RETRACKED: the relocalise's record and its count
    re->rv.flags = rl::RL_RETRACKED;
    fl = 0;
    CHECK(kfmr::measure_recover(true, key_prev, 1, *lost, 0, *re, 2, o, 10.0, z.get(), r_px.get(), m72.get(), fl) && fl == kfmr::FROM_RELOC);
    CHECK(kfm::relative_z(key_prev, other->px.offsets_px, z2.get()) && memcmp(z.get(), z2.get(), 32) == 0);
    fl = 0;
    CHECK(!kfmr::measure_recover(true, key_prev, 1, *lost, 2, *re, 0, o, 10.0, z.get(), r_px.get(), m72.get(), fl) && fl == kfm::NO_STEP);
    // ATTACHED: FIRST-like
    re->rv.flags = rl::RL_ATTACHED;
    fl = 0;
    CHECK(!kfmr::measure_recover(true, key_prev, 1, *lost, 2, *re, 2, o, 10.0, z.get(), r_px.get(), m72.get(), fl) && fl == kfmr::REATTACHED);
    // unrecovered
    lost->flags = kf::STOPPED | kf::BRIDGED | kf::REKEYED;
    re->rv.flags = rl::RL_NO_CANDIDATE;
    fl = 0;
    CHECK(!kfmr::measure_recover(true, key_prev, 1, *lost, 2, *re, 2, o, 10.0, z.get(), r_px.get(), m72.get(), fl) && fl == kfm::TRACK_LOST);
}

void whole_row(const Scene& scene, int capacity) {
    using photo_ref::NPIX;
    const std::vector<uint8_t> f0 = scene.view(0, 0), f1 = scene.view(2, -1), far = scene.view(64, -48), next = scene.view(66, -48), flat(NPIX, 93);
    std::vector<uint8_t> key(NPIX, 0), images((size_t)(capacity > 0 ? capacity : 1) * NPIX, 0);
    std::vector<km::Entry> e(capacity > 0 ? capacity : 1);
    memset(e.data(), 0, e.size() * sizeof(km::Entry));
    km::MapState ms = {0, 0, 0, 0};
    kfm::Session ks;
    memset(&ks, 0, sizeof ks);
    hnet_keyframe_measure_opts mo;
    hnet_keyframe_relocalise_opts ro;
    {
        kfm::Opts d;
        kfm::default_opts(d);
        d.cov_scale = 1.0;
        d.track.max_mse = 120.0;
        d.track.align.base.max_iterations = 6;
        memcpy(&mo, &d, sizeof mo);
        rl::Opts r;
        rl::default_opts(r);
        r.align.base.max_iterations = 6;
        memcpy(&ro, &r, sizeof ro);
    }
    std::vector<po::Hyp> tab(po::DEFAULT_COUNT);
    CHECK(po::yaw_table(po::DEFAULT_FIRST_DEG, po::DEFAULT_STEP_DEG, po::DEFAULT_COUNT, tab.data()));
    hnet_filter_params p;
    memset(&p, 0, sizeof p);
    p.c_R_i[0] = p.c_R_i[4] = p.c_R_i[8] = 1.0;
    p.gravity_mag = 9.81;
    p.k_net_cov = 10.0;
    float net72[72];
    memset(net72, 0, sizeof net72);
    for (int i = 0; i < 8; i++) net72[8 + i * 9] = 1.0f;
    const hnet_photo_residual script[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    std::unique_ptr<hnet_keyframe_measure_recover> out(new hnet_keyframe_measure_recover);
    double t = 1.0;
    auto call = [&](const std::vector<uint8_t>& f, float sx, float sy, int* counts) {
        hnet_filter_state st;
        memset(&st, 0, sizeof st);
        State s;
        memset(&s, 0, sizeof s);
        s.q[0] = 1.0;
        for (int c = 0; c < 4; c++) { s.offset[c][0] = sx / hnet_ekf::F_PIX; s.offset[c][1] = sy / hnet_ekf::F_PIX; }
        for (int i = 0; i < hnet_ekf::NS; i++) s.cov[i * hnet_ekf::NS + i] = 1e-4;
        st.t = t;
        t += 0.1;
        save(s, st);
        hnet_innovation inn[1];
        hnet_photo_residual prec[2];
        memset(out.get(), 0xA5, sizeof *out);
        return filters_keyframe_recover_ref_iterated(0, &st, &p, 1, net72, 0, 0.0, script, 0.0, 0, &mo, &ro, tab.data(), po::DEFAULT_COUNT, 0, &ks, key.data(), &ms,
                                                     e.data(), images.data(), capacity, f.data(), nullptr, 0, inn, prec, out.get(), counts);
    };
    int counts[3];
    CHECK(call(f0, 0, 0, counts) == 0 && out->m.flags == (kfm::ASKED | kfm::FIRST) && counts[2] == 0 && memcmp(key.data(), f0.data(), NPIX) == 0);
    CHECK(call(f1, 2, -1, counts) == 1 && out->m.flags == (kfm::ASKED | kfm::APPLIED) && counts[2] == 0 && out->reloc.target == rl::TARGET_NONE);
    if (capacity > 0) {
        CHECK(call(flat, 0, 0, counts) == 0 && out->m.flags == (kfm::ASKED | kfm::TRACK_LOST) && counts[2] == 1 && ks.prev_ok == 0);
        CHECK((out->m.track.flags & kf::REKEYED) && !(out->m.track.flags & kr::RECOVERED) && out->reloc.rv.flags == rl::RL_NO_CANDIDATE);
        CHECK(memcmp(key.data(), flat.data(), NPIX) == 0);
    }
    const int done = call(far, 0, 0, counts);
    printf("capacity %d: far frame: updates %d, flags %d, track flags %d, relocalise flags %d, nis %.1f\n", capacity, done, out->m.flags, out->m.track.flags,
           out->reloc.rv.flags, out->m.innov.nis);
    CHECK(counts[2] == 1 && (out->m.track.flags & kr::RECOVERED) && ks.prev_ok == 1);
    if (capacity > 0) {
        CHECK(done == 0 && out->m.flags == (kfm::ASKED | kfmr::REATTACHED) && out->reloc.rv.flags == rl::RL_ATTACHED && memcmp(key.data(), f0.data(), NPIX) == 0);
    } else {
        CHECK(done == 1 && out->m.flags == (kfm::ASKED | kfm::APPLIED | kfmr::FROM_RELOC) && out->reloc.rv.flags == rl::RL_RETRACKED);
        for (int k = 0; k < 8; k++) CHECK(std::fabs((double)out->m.z_px[k] - (k & 1 ? -48.0 + 1.0 : 64.0 - 2.0)) < 0.1);      // relative to the honest frame's key_px
    }
    CHECK(memcmp(ks.key.key_px, out->reloc.rv.key_px, sizeof ks.key.key_px) == 0);
    CHECK(call(next, 2, 0, counts) == 1 && out->m.flags == (kfm::ASKED | kfm::APPLIED) && counts[2] == 0);
    for (int k = 0; k < 8; k++) CHECK(std::fabs((double)out->m.z_px[k] - (k & 1 ? 0.0 : 2.0)) < 0.1);
}
}  // namespace

int main() {
    rule();
    const Scene scene;
    whole_row(scene, 0);
    whole_row(scene, 3);
    if (failures) { printf("filters keyframe recover check: %d FAILED\n", failures); return 1; }
    printf("filters keyframe recover check: ok\n");
    return 0;
}
