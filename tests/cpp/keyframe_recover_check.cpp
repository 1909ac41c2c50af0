// keyframe_recover_check.cpp — the shared functions of recovering a lost camera inside the track (include/hnet_keyframe_recover.h) and the host
// restatement of the whole call (tests/cpp/keyframe_recover_ref.cpp) on fixed inputs, meant for AddressSanitizer + UBSan on the CPU:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I <rocm>/include
//       -I cuahn_vio_amd/csrc -I include tests/cpp/keyframe_recover_check.cpp -o keyframe_recover_check && ./keyframe_recover_check
// The header's outcomes: a tracked frame, a first frame, and each LOST reason under each outcome of the relocalise and both values of auto_rekey, against
// the existing decide.  One whole row on heap frames of exactly 71 680 bytes, without a map and with one of 3 slots: a first frame, an honest frame, a
// frame (64, -48) px away tracked from a zero step (lost, found again on the held keyframe), the next frame with the true step, and with the map a
// constant frame (lost and unrecovered: the bridged re-key of the plain track).
// Exit status 0 = all hold.
#include "keyframe_recover_ref.cpp"

#include <cstdlib>

namespace {
int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

constexpr int CELL = 16, LW = 30, LH = 30, X0 = 72, Y0 = 120;      // lattice of 16-pixel cells covering 464 x 464

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
    // the view whose pixel (u, v) shows the scene at (u + X0 - dx, v + Y0 - dy): the keyframe's pixel x is seen at x + (dx, dy)
    std::vector<uint8_t> view(int dx, int dy) const {
        std::vector<uint8_t> f(photo_ref::NPIX);
        for (int v = 0; v < photo_ref::IMG_H; v++)
            for (int u = 0; u < photo_ref::IMG_W; u++) f[v * photo_ref::IMG_W + u] = at(u + X0 - dx, v + Y0 - dy);
        return f;
    }
};

kf::State held_state() {
    kf::State s;
    memset(&s, 0, sizeof s);
    s.has_key = 1; s.age = 2; s.keyframes = 3;
    for (int k = 0; k < 8; k++) s.key_px[k] = 1.0f + 0.25f * (float)k;
    for (int k = 0; k < 9; k++) s.h_origin_key[k] = (k & 3) == 0 ? 1.0 : 0.0;
    s.h_origin_key[2] = 12.0;
    return s;
}

hnet_robust::Record record(int flags, double mse, bool finite) {
    hnet_robust::Record r;
    memset(&r, 0, sizeof r);
    r.px.flags = flags; r.px.mse = mse; r.px.n_valid = 60000;
    for (int k = 0; k < 8; k++) r.px.offsets_px[k] = finite ? 2.0f + 0.5f * (float)k : NAN;
    return r;
}

bool same_tail(const kf::Track& a, const kf::Track& b) {
    return memcmp(a.start_px, b.start_px, sizeof a.start_px) == 0 && memcmp(a.key_px, b.key_px, sizeof a.key_px) == 0 &&
           memcmp(a.h_origin_curr, b.h_origin_curr, sizeof a.h_origin_curr) == 0 && a.overlap == b.overlap && a.age == b.age && a.keyframes == b.keyframes &&
           a.flags == b.flags && a.pad == b.pad;
}

void outcomes() {
    const float good[8] = {1.5f, 1.0f, 2.0f, 1.5f, 2.5f, 2.0f, 3.0f, 2.5f};
    float nan8[8];
    for (int k = 0; k < 8; k++) nan8[k] = kf::quiet_nan();
    struct Case { int why; const float* start; hnet_robust::Record rec; };
    const Case cases[4] = {{kf::NO_START, nan8, record(hnet_align::DEGENERATE, 0.0, true)}, {kf::STOPPED, good, record(hnet_align::SINGULAR, 5.0, true)},
                           {kf::MSE_ABOVE_MAX, good, record(0, 400.0, true)}, {kf::NON_FINITE, good, record(0, 5.0, false)}};
    const int results[9] = {rl::RL_RETRACKED, rl::RL_ATTACHED, rl::RL_NO_CANDIDATE, rl::RL_STOPPED, rl::RL_MSE_ABOVE_MAX, rl::RL_NON_FINITE, rl::RL_LOW_OVERLAP,
                            rl::RL_CLOSURE_ABOVE_MAX, rl::RL_CHAIN};
    for (int auto_rekey = 0; auto_rekey < 2; auto_rekey++) {
        kf::Opts o, o0;
        kf::default_opts(o);
        o.auto_rekey = auto_rekey; o.max_mse = 120.0;
        o0 = o; o0.auto_rekey = 0;
        // not lost, and a first frame: decide's own result, nothing active, a zero stash
        for (int first = 0; first < 2; first++) {
            kf::State s = held_state(), ns, n1;
            if (first) memset(&s, 0, sizeof s);
            kf::Track t, t1;
            memset(&t, 0, sizeof t);
            memset(&t1, 0, sizeof t1);
            kr::Stash st, zero;
            memset(&st, 0xA5, sizeof st);
            memset(&zero, 0, sizeof zero);
            int active = -1;
            const hnet_robust::Record r = record(0, 5.0, true);
            const int c = kr::decide_deferred(s, good, r, o, true, ns, t, st, active), c1 = kf::decide(s, good, r, o, true, n1, t1);
            CHECK(c == c1 && active == 0 && memcmp(&ns, &n1, sizeof ns) == 0 && same_tail(t, t1) && memcmp(&st, &zero, sizeof st) == 0);
            CHECK(first ? t.flags == (kf::FIRST | kf::REKEYED) : !kr::lost_of(t.flags));
        }
        for (const Case& cs : cases) {
            const kf::State s = held_state();
            kf::State s0, s1, ns;
            kf::Track t0, t1, t;
            memset(&t0, 0, sizeof t0); memset(&t1, 0, sizeof t1); memset(&t, 0, sizeof t);
            const int c0 = kf::decide(s, cs.start, cs.rec, o0, false, s0, t0), c1 = kf::decide(s, cs.start, cs.rec, o, false, s1, t1);
            kr::Stash st;
            memset(&st, 0xA5, sizeof st);
            int active = -1;
            const int c = kr::decide_deferred(s, cs.start, cs.rec, o, false, ns, t, st, active);
            CHECK(kr::lost_of(t0.flags) == cs.why && c0 == 0 && c1 == auto_rekey && c == 0 && active == 1);
            CHECK(memcmp(&ns, &s0, sizeof ns) == 0 && same_tail(t, t0) && memcmp(&st.state, &s1, sizeof s1) == 0 && st.copy == c1 && st.flags == t1.flags);
            for (int res : results) {
                kf::State left = ns;
                left.key_px[3] += 1.5f;
                left.age = 0;
                const kf::State was = left;
                kf::Track f = t;
                const int c2 = kr::finish(res, st, left, f);
                if (kr::recovered_by(res)) {
                    kf::Track want = t0;
                    want.flags |= kr::RECOVERED;
                    CHECK(c2 == 0 && memcmp(&left, &was, sizeof left) == 0 && same_tail(f, want));
                } else {
                    CHECK(c2 == c1 && memcmp(&left, &s1, sizeof left) == 0 && same_tail(f, t1));
                }
            }
        }
    }
    kr::Reloc z;
    memset(&z, 0xA5, sizeof z);
    kr::zero_reloc(z);
    CHECK(z.target == rl::TARGET_NONE && z.n_searched == 0 && z.rv.flags == 0 && z.search.hyp == 0 && z.pad == 0 && z.rv.rec.px.mse == 0.0);
}

void whole_row(const Scene& scene, int capacity) {
    using photo_ref::NPIX;
    const std::vector<uint8_t> f0 = scene.view(0, 0), f1 = scene.view(2, -1), far = scene.view(64, -48), next = scene.view(66, -48), flat(NPIX, 93);
    std::vector<uint8_t> key(NPIX, 0), images((size_t)(capacity > 0 ? capacity : 1) * NPIX, 0);
    std::vector<km::Entry> e(capacity > 0 ? capacity : 1);
    memset(e.data(), 0, e.size() * sizeof(km::Entry));
    km::MapState ms = {0, 0, 0, 0};
    kf::State s;
    memset(&s, 0, sizeof s);
    kr::Opts o;
    kr::default_opts(o);
    CHECK(o.track.max_mse == 0.0 && o.track.auto_rekey == 1 && o.reloc.levels == 4);
    o.track.max_mse = 120.0;
    o.track.align.base.max_iterations = 6;
    o.reloc.align.base.max_iterations = 6;
    std::vector<po::Hyp> tab(po::DEFAULT_COUNT);
    CHECK(po::yaw_table(po::DEFAULT_FIRST_DEG, po::DEFAULT_STEP_DEG, po::DEFAULT_COUNT, tab.data()));
    kr::Record out;
    kr::Reloc zero;
    kr::zero_reloc(zero);
    const float step1[8] = {2, -1, 2, -1, 2, -1, 2, -1}, step2[8] = {2, 0, 2, 0, 2, 0, 2, 0};
    auto call = [&](const std::vector<uint8_t>& f, const float* step) {
        return keyframe_recover_ref::track(s, key.data(), &ms, e.data(), images.data(), capacity, f.data(), step, o, tab.data(), po::DEFAULT_COUNT, false, nullptr,
                                           nullptr, out);
    };
    CHECK(call(f0, nullptr) == 0 && out.track.flags == (kf::FIRST | kf::REKEYED) && memcmp(&out.reloc, &zero, sizeof zero) == 0 && memcmp(key.data(), f0.data(), NPIX) == 0);
    CHECK(call(f1, step1) == 0 && !kr::lost_of(out.track.flags) && out.track.rec.px.mse * 3 < 120.0 && memcmp(&out.reloc, &zero, sizeof zero) == 0);
    if (capacity > 0) {
        // a constant frame: lost, nothing to find, the plain track's bridged re-key
        const kf::State before = s;
        kf::State twin = before;
        std::vector<uint8_t> twin_key(key);
        kf::Track tt;
        keyframe_ref_track(&twin, twin_key.data(), flat.data(), nullptr, &o.track, 0, &tt);
        CHECK(call(flat, nullptr) == 2 && kr::lost_of(out.track.flags) && (out.track.flags & kf::REKEYED) && !(out.track.flags & kr::RECOVERED));
        CHECK(out.reloc.rv.flags == rl::RL_NO_CANDIDATE && out.reloc.n_found == 0 && out.reloc.target == rl::TARGET_NONE);
        CHECK(memcmp(&out.track, &tt, sizeof tt) == 0 && memcmp(&s, &twin, sizeof s) == 0 && memcmp(key.data(), flat.data(), NPIX) == 0);
        printf("capacity %d: constant frame flags %d, searched %d; map cur_slot %d serial %d\n", capacity, out.track.flags, out.reloc.n_searched, ms.cur_slot, ms.serial);
    }
    const int what = call(far, nullptr);
    double worst = 0.0;
    for (int k = 0; k < 8; k++) worst = std::fmax(worst, std::fabs((double)out.reloc.rv.key_px[k] - (k & 1 ? -48.0 : 64.0)));
    printf("capacity %d: far frame: outcome %d, track flags %d (mse %.1f), relocalise flags %d, target %d, entry %d, worst corner error %.4f px\n", capacity, what,
           out.track.flags, out.track.rec.px.mse, out.reloc.rv.flags, out.reloc.target, out.reloc.search.hyp, worst);
    CHECK(what == 1 && kr::lost_of(out.track.flags) && (out.track.flags & kr::RECOVERED) && !(out.track.flags & kf::REKEYED));
    CHECK(kr::recovered_by(out.reloc.rv.flags) && out.reloc.n_found >= 1 && worst < 0.1);
    CHECK(capacity > 0 ? out.reloc.rv.flags == rl::RL_ATTACHED && out.reloc.target >= 0 && memcmp(key.data(), f0.data(), NPIX) == 0
                       : out.reloc.rv.flags == rl::RL_RETRACKED && out.reloc.target == rl::TARGET_HELD && (out.track.flags & kf::MSE_ABOVE_MAX));
    CHECK(memcmp(s.key_px, out.reloc.rv.key_px, sizeof s.key_px) == 0);
    CHECK(call(next, step2) == 0 && !kr::lost_of(out.track.flags) && !(out.track.flags & kr::RECOVERED) && memcmp(&out.reloc, &zero, sizeof zero) == 0);
    for (int k = 0; k < 8; k++) CHECK(std::fabs((double)out.track.key_px[k] - (k & 1 ? -48.0 : 66.0)) < 0.1);
}
}  // namespace

int main() {
    outcomes();
    const Scene scene;
    whole_row(scene, 0);
    whole_row(scene, 3);
    if (failures) { printf("keyframe_recover_check: %d FAILED\n", failures); return 1; }
    printf("keyframe_recover_check: ok\n");
    return 0;
}
