// photo_search_fine_check.cpp — the core of the fine stage's reference (tests/cpp/photo_search_fine_ref.cpp) and the shared functions
// (include/hnet_photo_search_fine.h) on fixed inputs, meant for AddressSanitizer + UBSan on the CPU:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I <rocm>/include
//       -I cuahn_vio_amd/csrc -I include tests/cpp/photo_search_fine_check.cpp -o photo_search_fine_check && ./photo_search_fine_check
// Heap level-2 thumbnails, warps and masks of exactly 4 480 bytes (an index one past either end is the sanitizer's to see): every shift at r = 4 at the four
// corners of the coarse range under the identity, a 45-degree and a scale-0.5 entry; a 9-entry row on a scene turned by 33 degrees; the hand-built kinds:
// a peak at level-2 shift (60, 40) whose shifts reach (64, 44), the same fine entry twice, a coarse record that is not FOUND, scale-0.5 entries that score
// nothing, a min_score of 1 on a near-match; and one fine relocalise of a session without a map.
// Exit status 0 = all hold.
#include "photo_search_fine_ref.cpp"

#include <cstdlib>

namespace {
int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

constexpr int CELL = 16, LW = 40, LH = 40;         // lattice of 16-pixel cells covering 624 x 624

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
    uint8_t at(double xd, double yd) const {
        const int x = (int)std::floor(xd), y = (int)std::floor(yd);
        if (x < 0 || y < 0 || x >= (LW - 1) * CELL || y >= (LH - 1) * CELL) return 0;
        const int x0 = x / CELL, y0 = y / CELL, fx = x % CELL, fy = y % CELL;
        const int top = lat[y0][x0] * (CELL - fx) + lat[y0][x0 + 1] * fx, bot = lat[y0 + 1][x0] * (CELL - fx) + lat[y0 + 1][x0 + 1] * fx;
        return (uint8_t)((top * (CELL - fy) + bot * fy) / (CELL * CELL));
    }
};

po::Record found(int hyp, int dx, int dy, const po::Hyp& h) {
    po::Record c;
    memset(&c, 0, sizeof c);
    c.base.flags = ps::FOUND; c.base.dx = dx; c.base.dy = dy; c.hyp = hyp;
    po::start_of(h.a, dx, dy, c.base.start_px);
    return c;
}

void check_part(const pf::Part& p, const po::Record& c, const po::Hyp* row, const pf::Opts& fo) {
    const int f = p.flags;
    CHECK(f == pf::FINE_REFINED || f == pf::FINE_SKIPPED || f == pf::FINE_NOTHING_SCORED || f == pf::FINE_LOW_SCORE);
    CHECK(p.pad0 == 0 && p.pad1 == 0 && p.j >= -1 && p.j < fo.n_fine && std::abs(p.ex) <= fo.radius && std::abs(p.ey) <= fo.radius);
    CHECK((p.j < 0) == (f == pf::FINE_SKIPPED || f == pf::FINE_NOTHING_SCORED));
    float want[8];
    if (f == pf::FINE_REFINED) pf::start_of(row[p.j].a, p.sx, p.sy, want);
    for (int k = 0; k < 8; k++)
        CHECK(f == pf::FINE_REFINED ? p.start_px[k] == want[k]
                                    : f == pf::FINE_SKIPPED ? std::isnan(p.start_px[k]) : memcmp(&p.start_px[k], &c.base.start_px[k], sizeof(float)) == 0);
    if (p.j >= 0) CHECK(p.sx == 2 * c.base.dx + p.ex && p.sy == 2 * c.base.dy + p.ey && p.n_overlap > 0 && p.score >= -1.0 && p.score <= 1.0);
    else CHECK(p.sx == 0 && p.sy == 0 && p.n_overlap == 0 && p.score == -1.0 && p.a[0] == 0.0 && p.sab == 0);
}
}  // namespace

int main() {
    using photo_ref::IMG_H;
    using photo_ref::IMG_W;
    using photo_ref::NPIX;
    const Scene scene;
    const double PI = std::acos(-1.0), yaw = 33.0 * PI / 180.0, tx = 24.0, ty = -16.0;
    // i2 is i1 turned by 33 degrees about the frame centre and moved by (tx, ty): i2(q) = scene(c + R^-1 (q - t - c))
    std::vector<uint8_t> i1(NPIX), i2(NPIX);
    for (int v = 0; v < IMG_H; v++)
        for (int u = 0; u < IMG_W; u++) {
            i1[v * IMG_W + u] = scene.at(u + 152.0, v + 200.0);
            const double qx = u - tx - po::CX, qy = v - ty - po::CY;
            i2[v * IMG_W + u] = scene.at(po::CX + std::cos(yaw) * qx + std::sin(yaw) * qy + 152.0, po::CY - std::sin(yaw) * qx + std::cos(yaw) * qy + 200.0);
        }
    std::vector<uint8_t> f1(pf::FPIX), f2(pf::FPIX), w(pf::FPIX), m(pf::FPIX), img(pf::FPIX), rnd(pf::FPIX);
    pf::thumbnail(i1.data(), f1.data());
    pf::thumbnail(i2.data(), f2.data());
    ps::Opts o;
    ps::default_opts(o);
    pf::Opts fo;
    pf::default_opts(fo);
    CHECK(pf::opts_valid(fo) && fo.radius == 3 && fo.n_fine == 5);
    { pf::Opts b = fo; b.radius = 5; CHECK(!pf::opts_valid(b)); b = fo; b.n_fine = 10; CHECK(!pf::opts_valid(b)); b = fo; b.min_score = NAN; CHECK(!pf::opts_valid(b)); }

    po::Hyp id, d45, half;
    CHECK(po::make_hyp(0.0, 1.0, id) && po::make_hyp(PI / 4, 1.0, d45) && po::make_hyp(0.0, 0.5, half));

    // every shift at r = 4 at the four corners of the coarse range under three entries
    const po::Hyp three[3] = {id, d45, half};
    for (int h = 0; h < 3; h++) {
        pf::warp_template(f1.data(), three[h].b, w.data(), m.data());
        int valid = 0;
        for (int k = 0; k < pf::FPIX; k++) { CHECK(m[k] <= 1 && (m[k] || w[k] == 0)); valid += m[k]; }
        printf("entry %d: %d valid template pixels\n", h, valid);
        CHECK(h == 0 ? valid == pf::FPIX && memcmp(w.data(), f1.data(), pf::FPIX) == 0 : valid > 0 && valid < pf::FPIX);
        if (h == 2) CHECK(valid == ps::TPIX);
        for (int cy = -1; cy <= 1; cy += 2)
            for (int cx = -1; cx <= 1; cx += 2)
                for (int ey = -pf::MAX_R; ey <= pf::MAX_R; ey++)
                    for (int ex = -pf::MAX_R; ex <= pf::MAX_R; ex++) {
                        const int sx = 2 * cx * ps::MAX_RX + ex, sy = 2 * cy * ps::MAX_RY + ey;
                        int u0, u1, v0, v1;
                        pf::overlap(sx, sy, u0, u1, v0, v1);
                        ps::Sums s;
                        pf::shift_sums(w.data(), m.data(), f2.data(), sx, sy, s);
                        CHECK(pf::shift_ok(sx, sy) && u1 > u0 && v1 > v0 && s.n >= 0 && s.n <= (u1 - u0) * (v1 - v0) && s.n <= valid && s.saa >= 0 && s.sbb >= 0);
                        if (h == 0) CHECK(s.n == (u1 - u0) * (v1 - v0));
                    }
    }
    // a 9-entry row around the 30-degree entry of a 12-degree table on the turned scene: the whole search of the two frames
    {
        std::vector<po::Hyp> tab(30), fine(30 * 9);
        CHECK(po::yaw_table(-180.0, 12.0, 30, tab.data()) && pf::fine_yaw_table(-180.0, 12.0, 30, 9, fine.data()) && pf::fine_table_valid(fine.data(), 30, 9));
        CHECK(memcmp(&fine[17 * 9 + 4], &tab[17], sizeof(po::Hyp)) == 0 && !pf::fine_yaw_table(-180.0, 12.0, 30, 10, fine.data()) && !pf::fine_table_valid(nullptr, 1, 1));
        pf::Opts f9 = fo;
        f9.n_fine = 9; f9.radius = 4;
        std::vector<double> scores((size_t)9 * pf::NSHIFT);
        pf::Record r;
        photo_search_fine_ref::search(i1.data(), i2.data(), o, tab.data(), 30, f9, fine.data(), r, nullptr, scores.data());
        printf("turned scene: coarse entry %d shift (%d, %d) score %.4f flags %d | fine j %d e (%d, %d) score %.4f flags %d start (%.2f, %.2f)\n", r.coarse.hyp,
               r.coarse.base.dx, r.coarse.base.dy, r.coarse.base.score, r.coarse.base.flags, r.fine.j, r.fine.ex, r.fine.ey, r.fine.score, r.fine.flags,
               r.fine.start_px[0], r.fine.start_px[1]);
        CHECK(r.coarse.base.flags == ps::FOUND && (r.coarse.hyp == 17 || r.coarse.hyp == 18) && r.fine.flags == pf::FINE_REFINED);
        check_part(r.fine, r.coarse, fine.data() + (size_t)r.coarse.hyp * 9, f9);
        CHECK(scores[(size_t)r.fine.j * pf::NSHIFT + (r.fine.ey + 4) * 9 + (r.fine.ex + 4)] == r.fine.score);
        // the truth at corner (0, 0): c + R (0 - c) + t
        const double gx = po::CX + std::cos(yaw) * -po::CX - std::sin(yaw) * -po::CY + tx, gy = po::CY + std::sin(yaw) * -po::CX + std::cos(yaw) * -po::CY + ty;
        const double ec = std::fmax(std::fabs(r.coarse.base.start_px[0] - gx), std::fabs(r.coarse.base.start_px[1] - gy));
        const double ef = std::fmax(std::fabs(r.fine.start_px[0] - gx), std::fabs(r.fine.start_px[1] - gy));
        printf("corner (0, 0): coarse start %.2f px from the truth, fine start %.2f px\n", ec, ef);
        CHECK(ef < ec);
    }
    // the hand-built kinds on the level-2 thumbnails
    {
        uint32_t s = 88172645u;
        for (int k = 0; k < pf::FPIX; k++) { s = s * 1664525u + 1013904223u; rnd[k] = (uint8_t)(s >> 24); }
        for (int k = 0; k < pf::FPIX; k++) { s = s * 1664525u + 1013904223u; img[k] = (uint8_t)(s >> 24); }
        for (int v = 40; v < pf::FH; v++)
            for (int u = 60; u < pf::FW; u++) img[v * pf::FW + u] = rnd[(v - 40) * pf::FW + (u - 60)];
        std::vector<double> scores((size_t)3 * pf::NSHIFT);
        pf::Part p;
        pf::Opts f1o = fo;
        f1o.n_fine = 1; f1o.radius = 4;
        po::Record c = found(0, 30, 20, id);
        pf::refine(rnd.data(), img.data(), c, 16, 1, f1o, &id, p, scores.data());
        check_part(p, c, &id, f1o);
        CHECK(p.flags == pf::FINE_REFINED && p.sx == 60 && p.sy == 40 && p.score == 1.0 && p.n_overlap == 320 && !std::isnan(scores[8 * 9 + 8]) && !std::isnan(scores[0]));
        // the same fine entry twice: the lower j wins
        const po::Hyp twice[3] = {d45, id, id};
        pf::Opts f3 = fo;
        f3.n_fine = 3; f3.radius = 2;
        c = found(0, 0, 0, id);
        pf::refine(f1.data(), f1.data(), c, o.min_overlap, 1, f3, twice, p, scores.data());
        check_part(p, c, twice, f3);
        CHECK(p.flags == pf::FINE_REFINED && p.j == 1 && p.ex == 0 && p.ey == 0 && p.score == 1.0 && scores[pf::NSHIFT + 40] == scores[2 * pf::NSHIFT + 40]);
        // a coarse record that is not FOUND, and a winner outside the table: SKIPPED, every score NaN
        po::Record low = c;
        low.base.flags = ps::LOW_SCORE;
        pf::refine(f1.data(), f1.data(), low, o.min_overlap, 1, f3, twice, p, scores.data());
        check_part(p, low, twice, f3);
        CHECK(p.flags == pf::FINE_SKIPPED && std::isnan(scores[40]));
        po::Record out_of_table = c;
        out_of_table.hyp = 1;
        pf::refine(f1.data(), f1.data(), out_of_table, o.min_overlap, 1, f3, twice, p, nullptr);
        CHECK(p.flags == pf::FINE_SKIPPED);
        // scale-0.5 entries at a min_overlap nothing meets: the coarse start is kept bit for bit
        const po::Hyp halves[2] = {half, half};
        pf::Opts f2o = fo;
        f2o.n_fine = 2;
        pf::refine(f1.data(), f1.data(), c, 300, 1, f2o, halves, p, scores.data());
        check_part(p, c, halves, f2o);
        CHECK(p.flags == pf::FINE_NOTHING_SCORED);
        // min_score 1 on a near-match
        std::vector<uint8_t> near(f1);
        near[10 * pf::FW + 20] ^= 1;
        pf::Opts one = f1o;
        one.min_score = 1.0; one.radius = 1;
        pf::refine(f1.data(), near.data(), c, o.min_overlap, 1, one, &id, p, scores.data());
        check_part(p, c, &id, one);
        CHECK(p.flags == pf::FINE_LOW_SCORE && p.j == 0 && p.ex == 0 && p.ey == 0 && p.score < 1.0 && p.score > 0.99);
    }
    // one fine relocalise of a session without a map: the keyframe is i1, the current frame i2
    {
        std::vector<po::Hyp> tab(30), fine(30 * 5);
        CHECK(po::yaw_table(-180.0, 12.0, 30, tab.data()) && pf::fine_yaw_table(-180.0, 12.0, 30, 5, fine.data()));
        kf::State st;
        memset(&st, 0, sizeof st);
        st.has_key = 1;
        for (int k = 0; k < 9; k++) st.h_origin_key[k] = (k & 3) == 0 ? 1.0 : 0.0;
        rl::Opts ro;
        rl::default_opts(ro);
        ro.min_overlap = 0.3;
        std::vector<uint8_t> key(i1);
        photo_search_fine_ref::Reloc out;
        const int attach = photo_search_fine_ref::relocalise(st, key.data(), nullptr, nullptr, nullptr, 0, i2.data(), ro, tab.data(), 30, fo, fine.data(), nullptr, out);
        printf("relocalise: target %d, searched %d, found %d, fine flags %d score %.4f, rv flags %d, overlap %.3f\n", out.base.target, out.base.n_searched,
               out.base.n_found, out.fine.flags, out.fine.score, out.base.rv.flags, out.base.rv.overlap);
        CHECK(attach == 0 && out.base.target == -1 && out.base.n_found == 1 && out.fine.flags == pf::FINE_REFINED);
        check_part(out.fine, out.base.search, fine.data() + (size_t)out.base.search.hyp * 5, fo);
        CHECK(memcmp(out.base.rv.start_px, out.fine.start_px, sizeof out.fine.start_px) == 0);
    }
    if (failures) { printf("photo_search_fine_check: %d FAILED\n", failures); return 1; }
    printf("photo_search_fine_check: ok\n");
    return 0;
}
