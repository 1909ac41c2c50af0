// photo_search_oriented_check.cpp — the core of the oriented search reference (tests/cpp/photo_search_oriented_ref.cpp) and the shared functions
// (include/hnet_photo_search_oriented.h) on fixed inputs, meant for AddressSanitizer + UBSan on the CPU:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I <rocm>/include
//       -I cuahn_vio_amd/csrc -I include tests/cpp/photo_search_oriented_check.cpp -o photo_search_oriented_check && ./photo_search_oriented_check
// Every shift of the full range under the identity, a 45-degree and a scale-0.5 entry on heap thumbnails of exactly 1 120 bytes (an index one past either
// end is the sanitizer's to see); a 64-entry table on a scene turned by a quarter and moved by (-24, 16) pixels; the hand-built cases: the same matrix
// twice, a scale-0.5 entry that scores nothing, a table of only such entries, a constant template, a peak at the edge of the radii under a 90-degree
// entry; and one oriented relocalise of a session without a map and with one, from the turned scene.
// Exit status 0 = all hold.
#include "photo_search_oriented_ref.cpp"

#include <cstdlib>

namespace {
int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

constexpr int CELL = 16, LW = 30, LH = 30, X0 = 72, Y0 = 120;      // lattice of 16-pixel cells covering 464 x 464; the frame's centre is (231.5, 231.5)

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
};

void check_record(const po::Record& r, const po::Hyp* hyps, int n_hyp) {
    const int f = r.base.flags;
    CHECK(f == ps::FOUND || f == ps::NO_TEXTURE || f == ps::LOW_SCORE || f == ps::AMBIGUOUS);
    CHECK(r.base.pad == 0 && r.pad0 == 0 && r.pad[0] == 0 && r.pad[1] == 0);
    CHECK(r.hyp >= -1 && r.hyp < n_hyp && r.hyp2 >= -1 && r.hyp2 < n_hyp && (r.hyp2 < 0 || r.hyp2 != r.hyp) && r.n_scored >= 0 && r.n_scored <= n_hyp);
    CHECK((r.hyp < 0) == (f == ps::NO_TEXTURE) && (r.hyp2 < 0) == (r.n_scored < 2) && r.score2 <= r.base.score);
    float want[8];
    if (f == ps::FOUND) po::start_of(hyps[r.hyp].a, r.base.dx, r.base.dy, want);
    for (int k = 0; k < 8; k++) CHECK(f == ps::FOUND ? r.base.start_px[k] == want[k] : std::isnan(r.base.start_px[k]));
    for (int k = 0; k < 4; k++) CHECK(r.a[k] == (r.hyp >= 0 ? hyps[r.hyp].a[k] : 0.0));
}
}  // namespace

int main() {
    using photo_ref::IMG_H;
    using photo_ref::IMG_W;
    using photo_ref::NPIX;
    const Scene scene;
    constexpr int DX = -24, DY = 16;
    // i2 is i1 turned by a quarter about the frame centre and moved by (DX, DY): the keyframe's pixel x is seen at c + R (x - c) + t, R = (0 -1; 1 0), so
    // i2(q) = scene(c + R^-1 (q - t - c)) = scene(qy - DY + 48, 271 - (qx - DX)) in frame coordinates
    std::vector<uint8_t> i1(NPIX), i2(NPIX), white(NPIX, 255);
    for (int v = 0; v < IMG_H; v++)
        for (int u = 0; u < IMG_W; u++) {
            i1[v * IMG_W + u] = scene.at(u + X0, v + Y0);
            i2[v * IMG_W + u] = scene.at((v - DY + 48) + X0, (271 - (u - DX)) + Y0);
        }
    // heap thumbnails, warps and masks of exactly TPIX bytes
    std::vector<uint8_t> t1(ps::TPIX), t2(ps::TPIX), w(ps::TPIX), m(ps::TPIX), flat(ps::TPIX, 93), tall(ps::TPIX), edge(ps::TPIX);
    ps::thumbnail(i1.data(), t1.data());
    ps::thumbnail(i2.data(), t2.data());
    ps::Opts o;
    ps::default_opts(o);

    // tables: make_hyp's limits, and what a call refuses
    po::Hyp id, q90, d45, half, bad;
    CHECK(po::make_hyp(0.0, 1.0, id) && po::make_hyp(std::acos(-1.0) / 2, 1.0, q90) && po::make_hyp(std::acos(-1.0) / 4, 1.0, d45) && po::make_hyp(0.0, 0.5, half));
    CHECK(!po::make_hyp(0.0, 0.49, bad) && !po::make_hyp(0.0, 2.01, bad) && !po::make_hyp(NAN, 1.0, bad) && !po::make_hyp(0.0, NAN, bad));
    CHECK(id.b[0] == po::ONE && id.b[1] == 0 && id.b[2] == 0 && id.b[3] == po::ONE && q90.b[0] == 0 && q90.b[1] == po::ONE && q90.b[2] == -po::ONE && q90.b[3] == 0);
    CHECK(half.b[0] == po::MAX_B && po::hyp_valid(half));
    bad = id; bad.b[2] = po::MAX_B + 1; CHECK(!po::hyp_valid(bad));
    bad = id; bad.a[3] = INFINITY; CHECK(!po::hyp_valid(bad));
    CHECK(!po::table_valid(&id, 0) && !po::table_valid(&id, 65) && !po::table_valid(nullptr, 1) && po::table_valid(&id, 1));

    // every shift of the full range under three entries: the identity's sums are 7r's, no entry counts more than the overlap
    const po::Hyp three[3] = {id, d45, half};
    for (int h = 0; h < 3; h++) {
        po::warp_template(t1.data(), three[h].b, w.data(), m.data());
        int valid = 0;
        for (int k = 0; k < ps::TPIX; k++) { CHECK(m[k] <= 1 && (m[k] || w[k] == 0)); valid += m[k]; }
        printf("entry %d: %d valid template pixels\n", h, valid);
        CHECK(h == 0 ? valid == ps::TPIX && memcmp(w.data(), t1.data(), ps::TPIX) == 0 : valid > 0 && valid < ps::TPIX);
        for (int i = 0; i < ps::NSHIFT; i++) {
            int dx, dy;
            ps::index_shift(i, dx, dy);
            ps::Sums s, p;
            po::shift_sums(w.data(), m.data(), t2.data(), dx, dy, s);
            ps::shift_sums(t1.data(), t2.data(), dx, dy, p);
            CHECK(s.n >= 0 && s.n <= p.n && s.n <= valid && s.sb <= p.sb && s.sbb <= p.sbb && s.saa < (1 << 27));
            if (h == 0) CHECK(memcmp(&s, &p, sizeof s) == 0);
        }
    }
    // a 64-entry table on the turned scene: entry 48 of 5.625 degrees from -180 is the quarter turn
    {
        std::vector<po::Hyp> tab(po::MAX_HYP);
        CHECK(po::yaw_table(-180.0, 5.625, po::MAX_HYP, tab.data()) && !po::yaw_table(-180.0, 6.0, 65, tab.data()) && !po::yaw_table(NAN, 6.0, 4, tab.data()));
        std::vector<double> scores((size_t)po::MAX_HYP * ps::NSHIFT);
        std::vector<ps::Record> per(po::MAX_HYP);
        po::Record r;
        po::search(t1.data(), t2.data(), o, tab.data(), po::MAX_HYP, r, scores.data(), per.data());
        printf("turned scene: entry %d, shift (%d, %d), score %.4f, second %.4f, runner-up entry %d at %.4f, %d entries scored, flags %d\n", r.hyp, r.base.dx,
               r.base.dy, r.base.score, r.base.second, r.hyp2, r.score2, r.n_scored, r.base.flags);
        check_record(r, tab.data(), po::MAX_HYP);
        CHECK(r.hyp == 48 && r.base.dx == DX / 8 && r.base.dy == DY / 8 && r.base.flags == ps::FOUND && r.n_scored == po::MAX_HYP);
        CHECK(scores[(size_t)r.hyp * ps::NSHIFT + ps::shift_index(r.base.dx, r.base.dy)] == r.base.score && per[r.hyp2].score == r.score2);
        ps::Record plain;
        ps::search(t1.data(), t2.data(), o, plain, scores.data());
        CHECK(plain.flags != ps::FOUND);
        // the identity alone is 7r's record
        po::search(t1.data(), t2.data(), o, &id, 1, r, scores.data(), nullptr);
        CHECK(memcmp(&r.base, &plain, sizeof plain) == 0 && r.hyp2 == -1 && r.score2 == -1.0);
    }
    // the hand-built cases
    {
        po::Record r;
        const po::Hyp twice[3] = {d45, id, id};
        po::search(t1.data(), t1.data(), o, twice, 3, r, nullptr, nullptr);
        check_record(r, twice, 3);
        CHECK(r.hyp == 1 && r.hyp2 == 2 && r.score2 == r.base.score && r.base.score == 1.0 && r.base.dx == 0 && r.base.dy == 0);
        ps::Opts z = o;
        z.min_overlap = 300;                                               // a scale of 0.5 leaves 20 x 14 valid pixels
        const po::Hyp mixed[2] = {half, id}, halves[2] = {half, half};
        po::search(t1.data(), t1.data(), z, mixed, 2, r, nullptr, nullptr);
        check_record(r, mixed, 2);
        CHECK(r.hyp == 1 && r.hyp2 == -1 && r.n_scored == 1 && r.base.flags == ps::FOUND);
        po::search(t1.data(), t1.data(), z, halves, 2, r, nullptr, nullptr);
        check_record(r, halves, 2);
        CHECK(r.base.flags == ps::NO_TEXTURE && r.hyp == -1 && r.n_scored == 0 && r.base.score == -1.0 && r.base.n_overlap == 0);
        const po::Hyp some[3] = {id, q90, d45};
        po::search(flat.data(), t1.data(), o, some, 3, r, nullptr, nullptr);
        check_record(r, some, 3);
        CHECK(r.base.flags == ps::NO_TEXTURE && r.hyp == -1);
        // a peak at (30, 20) under the quarter turn: the warp of `tall` is valid on columns 6 .. 33; the overlap of the shift is columns 6 .. 9, rows 0 .. 7
        uint32_t s = 88172645u;
        for (int k = 0; k < ps::TPIX; k++) { s = s * 1664525u + 1013904223u; tall[k] = (uint8_t)(s >> 24); }
        for (int k = 0; k < ps::TPIX; k++) { s = s * 1664525u + 1013904223u; edge[k] = (uint8_t)(s >> 24); }
        po::warp_template(tall.data(), q90.b, w.data(), m.data());
        for (int v = 0; v < ps::TH; v++)
            for (int u = 0; u < ps::TW; u++) {
                CHECK(m[v * ps::TW + u] == (u >= 6 && u <= 33 ? 1 : 0));
                if (m[v * ps::TW + u]) CHECK(w[v * ps::TW + u] == tall[(33 - u) * ps::TW + (v + 6)]);
            }
        for (int v = 0; v < ps::TH - 20; v++)
            for (int u = 0; u < ps::TW - 30; u++) edge[(v + 20) * ps::TW + (u + 30)] = w[v * ps::TW + u];
        z = o;
        z.min_overlap = 32;
        const po::Hyp two[2] = {id, q90};
        po::search(tall.data(), edge.data(), z, two, 2, r, nullptr, nullptr);
        check_record(r, two, 2);
        CHECK(r.hyp == 1 && r.base.dx == 30 && r.base.dy == 20 && r.base.n_overlap == 32 && std::fabs(r.base.score - 1.0) < 1e-15);
    }
    // one oriented relocalise without a map and one with: the session holds i1 as its keyframe with a key_px far from the truth
    {
        const po::Hyp tab[3] = {id, d45, q90};
        float truth[8];
        po::start_of(q90.a, DX / 8, DY / 8, truth);
        rl::Opts ro;
        rl::default_opts(ro);
        ro.align.base.max_iterations = 6;
        kf::State s;
        memset(&s, 0, sizeof s);
        s.has_key = 1; s.keyframes = 1; s.age = 1;
        for (int k = 0; k < 9; k++) s.h_origin_key[k] = (k & 3) == 0 ? 1.0 : 0.0;
        std::vector<uint8_t> key(i1);
        rl::Reloc plain;
        int attach = photo_search_ref::relocalise(s, key.data(), nullptr, nullptr, nullptr, 0, i2.data(), ro, nullptr, plain);
        CHECK(attach == 0 && plain.rv.flags == rl::RL_NO_CANDIDATE);
        photo_search_oriented_ref::Reloc out;
        attach = photo_search_oriented_ref::relocalise(s, key.data(), nullptr, nullptr, nullptr, 0, i2.data(), ro, tab, 3, nullptr, out);
        double worst = 0.0;
        for (int k = 0; k < 8; k++) worst = std::fmax(worst, std::fabs((double)out.rv.key_px[k] - (double)truth[k]));
        printf("relocalise, no map: flags %d, target %d, entry %d, searched %d, found %d, worst corner error %.4f px\n", out.rv.flags, out.target, out.search.hyp,
               out.n_searched, out.n_found, worst);
        CHECK(attach == 0 && out.rv.flags == rl::RL_RETRACKED && out.target == rl::TARGET_HELD && out.search.hyp == 2 && out.n_searched == 1 && out.n_found == 1 &&
              worst < 0.1);
        CHECK(memcmp(s.key_px, out.rv.key_px, sizeof s.key_px) == 0 && s.age == 1 && s.keyframes == 1);
        // with a map of 3 slots: slot 0 holds i1, the held keyframe is a constant frame in slot 1 (cur_slot), slot 2 is invalid
        constexpr int M = 3;
        std::vector<uint8_t> images((size_t)M * NPIX, 93);
        memcpy(images.data(), i1.data(), NPIX);
        km::Entry e[M];
        memset(e, 0, sizeof e);
        for (int i = 0; i < 2; i++) {
            e[i].valid = 1; e[i].links = i; e[i].serial = i + 1;
            for (int k = 0; k < 9; k++) e[i].h_origin_key[k] = (k & 3) == 0 ? 1.0 : 0.0;
        }
        e[1].h_origin_key[2] = 50.0;                                       // the chain believes the held keyframe lies 50 px away
        km::MapState ms = {1, 1, 1, 2};
        memset(&s, 0, sizeof s);
        s.has_key = 1; s.keyframes = 2; s.age = 1;
        memcpy(s.h_origin_key, e[1].h_origin_key, sizeof s.h_origin_key);
        std::fill(key.begin(), key.end(), 93);
        attach = photo_search_oriented_ref::relocalise(s, key.data(), &ms, e, images.data(), M, i2.data(), ro, tab, 3, nullptr, out);
        printf("relocalise, map: flags %d, target %d, entry %d, searched %d, found %d\n", out.rv.flags, out.target, out.search.hyp, out.n_searched, out.n_found);
        CHECK(attach == 1 && out.rv.flags == rl::RL_ATTACHED && out.target == 0 && out.search.hyp == 2 && out.n_searched == 2 && out.n_found == 1 && ms.cur_slot == 0);
        CHECK(memcmp(key.data(), i1.data(), NPIX) == 0 && s.age == 0);
        // an unrelated (constant) current frame: nothing is found and nothing changes
        const kf::State keep = s;
        const km::MapState mkeep = ms;
        attach = photo_search_oriented_ref::relocalise(s, key.data(), &ms, e, images.data(), M, white.data(), ro, tab, 3, nullptr, out);
        CHECK(attach == 0 && out.rv.flags == rl::RL_NO_CANDIDATE && out.target == rl::TARGET_NONE && out.n_found == 0 && out.search.hyp == 0 && out.search.a[0] == 0.0);
        CHECK(memcmp(&keep, &s, sizeof s) == 0 && memcmp(&mkeep, &ms, sizeof ms) == 0);
    }
    if (failures) { printf("photo_search_oriented_check: %d FAILED\n", failures); return 1; }
    printf("photo_search_oriented_check: ok\n");
    return 0;
}
