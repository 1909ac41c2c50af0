// photo_search_check.cpp — the core of the search reference (tests/cpp/photo_search_ref.cpp) and the shared functions (include/hnet_photo_search.h,
// include/hnet_keyframe_reloc.h) on fixed inputs, meant for AddressSanitizer + UBSan on the CPU:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I <rocm>/include
//       -I cuahn_vio_amd/csrc -I include tests/cpp/photo_search_check.cpp -o photo_search_check && ./photo_search_check
// The thumbnail of a fixed scene against level 3 of the pyramid reference, of a 0 / 255 checker frame and of an all-255 frame; every shift of the full
// range on heap thumbnails of exactly 1 120 bytes (an index one past either end is the sanitizer's to see); a scene moved by (-24, 16) pixels found at
// (-3, 2); the hostile thumbnails: constant (NO_TEXTURE), a 0 / 255 checker (AMBIGUOUS), radius 0, the corners of the range, a min_overlap that excludes
// everything but the centre; and one relocalise of a session without a map and with one, from the moved scene.
// Exit status 0 = all hold.
#include "photo_search_ref.cpp"

#include <cstdlib>

namespace {
int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

constexpr int CELL = 16, LW = 26, LH = 20, MARGIN = 40;      // lattice of 16-pixel cells covering 400 x 304

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

void check_record(const ps::Record& r) {
    const int f = r.flags;
    CHECK(f == ps::FOUND || f == ps::NO_TEXTURE || f == ps::LOW_SCORE || f == ps::AMBIGUOUS);
    CHECK(r.pad == 0 && r.dx >= -ps::MAX_RX && r.dx <= ps::MAX_RX && r.dy >= -ps::MAX_RY && r.dy <= ps::MAX_RY);
    CHECK(r.score >= -1.0000001 && r.score <= 1.0000001 && r.second >= -1.0000001 && r.second <= r.score);
    for (int k = 0; k < 8; k++) CHECK(f == ps::FOUND ? r.start_px[k] == (float)(8 * (k % 2 ? r.dy : r.dx)) : std::isnan(r.start_px[k]));
}
}  // namespace

int main() {
    using photo_ref::IMG_H;
    using photo_ref::IMG_W;
    using photo_ref::NPIX;
    const Scene scene;
    constexpr int DX = -24, DY = 16;
    std::vector<uint8_t> i1(NPIX), i2(NPIX), white(NPIX, 255), checker(NPIX);
    for (int v = 0; v < IMG_H; v++)
        for (int u = 0; u < IMG_W; u++) {
            i1[v * IMG_W + u] = scene.at(u + MARGIN, v + MARGIN);
            i2[v * IMG_W + u] = scene.at(u + MARGIN - DX, v + MARGIN - DY);      // img2(x + (DX, DY)) = img1(x)
            checker[v * IMG_W + u] = ((u + v) & 1) ? 255 : 0;
        }
    // heap thumbnails of exactly TPIX bytes
    std::vector<uint8_t> t1(ps::TPIX), t2(ps::TPIX), tw(ps::TPIX), tc(ps::TPIX), flat(ps::TPIX, 93), chk(ps::TPIX);
    std::vector<double> scores(ps::NSHIFT);
    ps::Opts o;
    ps::default_opts(o);
    CHECK(ps::opts_valid(o));

    // the thumbnail is level 3 of the pyramid reference
    {
        std::vector<uint8_t> packed(hnet_align::PYR_BYTES);
        photo_align_pyr_ref_pyramid(i1.data(), 1, packed.data());
        ps::thumbnail(i1.data(), t1.data());
        ps::thumbnail(i2.data(), t2.data());
        ps::thumbnail(white.data(), tw.data());
        ps::thumbnail(checker.data(), tc.data());
        CHECK(memcmp(t1.data(), packed.data() + hnet_align::level_offset(3), ps::TPIX) == 0);
        for (int k = 0; k < ps::TPIX; k++) CHECK(tw[k] == 255 && tc[k] == 128);
    }
    // every shift of the full range: the overlap is never empty, the sums stay below 2^27
    for (int i = 0; i < ps::NSHIFT; i++) {
        int dx, dy;
        ps::index_shift(i, dx, dy);
        CHECK(ps::shift_index(dx, dy) == i);
        ps::Sums s;
        ps::shift_sums(t1.data(), tw.data(), dx, dy, s);
        CHECK(s.n == (ps::TW - abs(dx)) * (ps::TH - abs(dy)) && s.n >= 80 && s.sb == 255 * s.n && s.sbb == 255 * 255 * s.n && s.saa < (1 << 27));
    }
    // the moved scene
    {
        ps::Record r;
        ps::search(t1.data(), t2.data(), o, r, scores.data());
        printf("moved scene: shift (%d, %d), score %.4f, second %.4f at (%d, %d), flags %d\n", r.dx, r.dy, r.score, r.second, r.dx2, r.dy2, r.flags);
        check_record(r);
        CHECK(r.dx == DX / 8 && r.dy == DY / 8 && r.flags == ps::FOUND && r.n_overlap == (ps::TW - 3) * (ps::TH - 2));
        CHECK(scores[ps::shift_index(r.dx, r.dy)] == r.score && scores[ps::shift_index(r.dx2, r.dy2)] == r.second);
    }
    // hostile thumbnails
    {
        ps::Record r;
        for (int k = 0; k < ps::TPIX; k++) chk[k] = ((k % ps::TW + k / ps::TW) & 1) ? 255 : 0;
        ps::search(t1.data(), flat.data(), o, r, scores.data());
        check_record(r);
        CHECK(r.flags == ps::NO_TEXTURE && r.score == -1.0 && r.n_overlap == 0 && r.sab == 0);
        for (int i = 0; i < ps::NSHIFT; i++) CHECK(std::isnan(scores[i]));
        ps::search(flat.data(), t1.data(), o, r, scores.data());
        CHECK(r.flags == ps::NO_TEXTURE);
        ps::search(chk.data(), chk.data(), o, r, scores.data());
        check_record(r);
        CHECK(r.flags == ps::AMBIGUOUS && r.dx == 0 && r.dy == 0 && r.score == 1.0 && r.second == 1.0 && r.dx2 == 0 && r.dy2 == -2);
        ps::Opts z = o;
        z.radius_x = z.radius_y = 0;
        ps::search(t1.data(), t1.data(), z, r, scores.data());
        check_record(r);
        CHECK(r.flags == ps::FOUND && r.dx == 0 && r.dy == 0 && r.second == -1.0 && r.n_overlap == ps::TPIX);
        int scored = 0;
        for (int i = 0; i < ps::NSHIFT; i++) scored += std::isnan(scores[i]) ? 0 : 1;
        CHECK(scored == 1);
        // the corners of the range are scored at min_overlap 16 and not at the default; min_overlap 1120 leaves the centre alone
        z = o;
        z.min_overlap = ps::MIN_MIN_OVERLAP;
        ps::search(t1.data(), t2.data(), z, r, scores.data());
        check_record(r);
        CHECK(!std::isnan(scores[0]) && !std::isnan(scores[ps::NSHIFT - 1]) && !std::isnan(scores[ps::NSX - 1]) && !std::isnan(scores[ps::NSHIFT - ps::NSX]));
        ps::search(t1.data(), t2.data(), o, r, scores.data());
        CHECK(std::isnan(scores[0]) && std::isnan(scores[ps::NSHIFT - 1]));
        z.min_overlap = ps::TPIX;
        ps::search(t1.data(), t2.data(), z, r, scores.data());
        check_record(r);
        CHECK(r.dx == 0 && r.dy == 0 && r.second == -1.0);
        z.min_overlap = ps::TPIX + 1;
        CHECK(!ps::opts_valid(z));
        z = o; z.radius_x = 31; CHECK(!ps::opts_valid(z));
        z = o; z.min_score = NAN; CHECK(!ps::opts_valid(z));
        z = o; z.min_margin = -0.1; CHECK(!ps::opts_valid(z));
    }
    // one relocalise without a map and one with: the session holds i1 as its keyframe with a key_px far from the truth
    {
        rl::Opts ro;
        rl::default_opts(ro);
        ro.align.base.max_iterations = 6;
        CHECK(rl::opts_valid(ro));
        kf::State s;
        memset(&s, 0, sizeof s);
        s.has_key = 1; s.keyframes = 1; s.age = 1;
        for (int k = 0; k < 9; k++) s.h_origin_key[k] = (k & 3) == 0 ? 1.0 : 0.0;
        std::vector<uint8_t> key(i1);
        rl::Reloc out;
        int attach = photo_search_ref::relocalise(s, key.data(), nullptr, nullptr, nullptr, 0, i2.data(), ro, nullptr, out);
        double worst = 0.0;
        for (int k = 0; k < 8; k++) worst = std::fmax(worst, std::fabs((double)out.rv.key_px[k] - (k % 2 ? DY : DX)));
        printf("relocalise, no map: flags %d, target %d, searched %d, found %d, worst corner error %.4f px\n", out.rv.flags, out.target, out.n_searched, out.n_found, worst);
        CHECK(attach == 0 && out.rv.flags == rl::RL_RETRACKED && out.target == rl::TARGET_HELD && out.n_searched == 1 && out.n_found == 1 && worst < 0.1);
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
        km::MapState m = {1, 1, 1, 2};
        memset(&s, 0, sizeof s);
        s.has_key = 1; s.keyframes = 2; s.age = 1;
        memcpy(s.h_origin_key, e[1].h_origin_key, sizeof s.h_origin_key);
        std::fill(key.begin(), key.end(), 93);
        attach = photo_search_ref::relocalise(s, key.data(), &m, e, images.data(), M, i2.data(), ro, nullptr, out);
        printf("relocalise, map: flags %d, target %d, searched %d, found %d\n", out.rv.flags, out.target, out.n_searched, out.n_found);
        CHECK(attach == 1 && out.rv.flags == rl::RL_ATTACHED && out.target == 0 && out.n_searched == 2 && out.n_found == 1 && m.cur_slot == 0 && m.cur_links == 0);
        CHECK(memcmp(key.data(), i1.data(), NPIX) == 0 && s.h_origin_key[2] == 0.0 && s.age == 0);
        // an unrelated (constant) current frame: nothing is found and nothing changes
        const kf::State keep = s;
        const km::MapState mkeep = m;
        attach = photo_search_ref::relocalise(s, key.data(), &m, e, images.data(), M, white.data(), ro, nullptr, out);
        CHECK(attach == 0 && out.rv.flags == rl::RL_NO_CANDIDATE && out.target == rl::TARGET_NONE && out.n_found == 0);
        CHECK(memcmp(&keep, &s, sizeof s) == 0 && memcmp(&mkeep, &m, sizeof m) == 0);
    }
    if (failures) { printf("photo_search_check: %d FAILED\n", failures); return 1; }
    printf("photo_search_check: ok\n");
    return 0;
}
