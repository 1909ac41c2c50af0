// photo_masked_check.cpp — the masked alignment's host reference (tests/cpp/photo_masked_ref.cpp) and the functions of include/hnet_photo_masked.h on fixed
// inputs, meant for AddressSanitizer + UBSan on the CPU:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I <rocm>/include
//       -I cuahn_vio_amd/csrc -I include tests/cpp/photo_masked_check.cpp -o photo_masked_check && ./photo_masked_check
// A fixed scene moved by (6, -4) pixels.  Hostile masks (none, one byte, the last byte alone, the last row and column, a checkerboard, noise, bands, all)
// against hostile starts (zero, NaN with a payload, 400 px away, four corners on a line, 1e30) with min_valid 0 and the default: the pyramid and its counts
// against a direct count, a full mask against the robust reference byte for byte, an empty one FEW_PIXELS with nothing valid, and a half mask that hides
// a block of noise in img1 finding the move as if the block were not there.  Then the localise rule (tests/cpp/keyframe_localise_ref.cpp) on hostile entries,
// masks, counts, records, states and options.
// Exit status 0 = all hold.
#include "keyframe_localise_ref.cpp"      // (includes photo_masked_ref.cpp)

#include <cstdlib>

namespace {
int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

constexpr int CELL = 16, LW = 26, LH = 20, MARGIN = 40;      // lattice of 16-pixel cells covering 400 x 304

// photo_robust_check.cpp's fixed smooth scene: bilinear interpolation of an LCG lattice
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
}  // namespace

int main() {
    using photo_ref::IMG_H;
    using photo_ref::IMG_W;
    using photo_ref::NPIX;
    namespace pa = hnet_align;
    namespace pr = hnet_robust;
    namespace pm = hnet_masked;
    const Scene scene;
    constexpr int DX = 6, DY = -4;
    std::vector<uint8_t> i1(NPIX), i2(NPIX), spoiled(NPIX);
    uint32_t s = 88172645u;
    for (int v = 0; v < IMG_H; v++)
        for (int u = 0; u < IMG_W; u++) {
            i1[v * IMG_W + u] = scene.at(u + MARGIN, v + MARGIN);
            i2[v * IMG_W + u] = scene.at(u + MARGIN - DX, v + MARGIN - DY);      // img2(x + (DX, DY)) = img1(x)
            s = s * 1664525u + 1013904223u;
            spoiled[v * IMG_W + u] = u >= 160 ? (uint8_t)(s >> 24) : i1[v * IMG_W + u];      // the right half of img1 is noise
        }

    // the masks
    struct Mask { const char* name; std::vector<uint8_t> m; };
    std::vector<Mask> masks;
    masks.push_back({"none", std::vector<uint8_t>(NPIX, 0)});
    masks.push_back({"all", std::vector<uint8_t>(NPIX, 255)});
    masks.push_back({"first byte", std::vector<uint8_t>(NPIX, 0)});
    masks.back().m[0] = 1;
    masks.push_back({"last byte", std::vector<uint8_t>(NPIX, 0)});
    masks.back().m[NPIX - 1] = 128;
    masks.push_back({"last row and column", std::vector<uint8_t>(NPIX, 0)});
    for (int u = 0; u < IMG_W; u++) masks.back().m[(IMG_H - 1) * IMG_W + u] = 255;
    for (int v = 0; v < IMG_H; v++) masks.back().m[v * IMG_W + IMG_W - 1] = 255;
    masks.push_back({"checkerboard", std::vector<uint8_t>(NPIX, 0)});
    for (int p = 0; p < NPIX; p++) masks.back().m[p] = (uint8_t)((((p % IMG_W) + (p / IMG_W)) & 1) * 255);
    masks.push_back({"noise", std::vector<uint8_t>(NPIX, 0)});
    for (int p = 0; p < NPIX; p++) { s = s * 1664525u + 1013904223u; masks.back().m[p] = (uint8_t)((s >> 24) & 0x83u); }
    masks.push_back({"left half", std::vector<uint8_t>(NPIX, 0)});
    for (int p = 0; p < NPIX; p++) masks.back().m[p] = (p % IMG_W) < 160 ? 7 : 0;
    masks.push_back({"rows 96 on", std::vector<uint8_t>(NPIX, 255)});
    memset(masks.back().m.data(), 0, 96 * IMG_W);

    // the pyramid and its counts against a direct count of the 4^L bytes under every pixel
    for (const Mask& mk : masks) {
        std::vector<uint8_t> pyr(pa::PYR_BYTES, 0xA5);
        int32_t n_mask[pm::N_MASK];
        pm::mask_pyramid(mk.m.data(), pyr.data());
        pm::mask_counts(mk.m.data(), pyr.data(), n_mask);
        for (int L = 0; L < pa::MAX_LEVELS; L++) {
            const uint8_t* lv = pm::mask_level(mk.m.data(), pyr.data(), L);
            const int sc = 1 << L, w = pa::level_w(L), h = pa::level_h(L);
            int counts[pm::SLICES] = {0, 0, 0, 0, 0, 0, 0};
            for (int v = 0; v < h; v++)
                for (int u = 0; u < w; u++) {
                    bool all = true;
                    for (int dv = 0; dv < sc; dv++)
                        for (int du = 0; du < sc; du++) all = all && mk.m[(v * sc + dv) * IMG_W + u * sc + du] != 0;
                    CHECK(pm::takes_part(lv, L, u, v) == all);
                    if (L > 0) CHECK(lv[v * w + u] == (all ? 1 : 0));
                    counts[v / pm::slice_rows(L)] += all ? 1 : 0;
                }
            for (int k = 0; k < pm::SLICES; k++) CHECK(n_mask[L * pm::SLICES + k] == counts[k]);
        }
    }

    // every mask against every start, min_valid 0 and the default
    const float big = 1e30f;
    float line[8] = {0, 0, 10, 5, 20, 10, 30, 15}, far[8], nanp[8] = {0, 0, 0, 0, 0, 0, 0, 0}, zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float huge[8] = {big, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 8; k++) { line[k] -= (float)hnet::p4(k); far[k] = k % 2 ? 0.0f : 400.0f; }
    const uint32_t payload = 0x7FC12345u;
    memcpy(&nanp[3], &payload, 4);
    const float* starts[] = {zero, nanp, far, line, huge};
    for (int mv = 0; mv <= 20000; mv += 20000)
        for (const Mask& mk : masks)
            for (const float* x0 : starts) {
                pr::Opts o;
                pr::default_opts(o);
                o.base.max_iterations = 6;
                o.base.min_valid = mv;
                pr::Record recs[pa::MAX_LEVELS], want[pa::MAX_LEVELS];
                memset(recs, 0, sizeof recs);
                memset(want, 0, sizeof want);
                photo_masked_ref::align(i1.data(), mk.m.data(), i2.data(), x0, o, 4, recs);
                int total = 0;
                for (int p = 0; p < NPIX; p++) total += mk.m[p] != 0;
                for (int L = 0; L < 4; L++) {
                    CHECK(recs[L].px.n_valid0 >= 0 && recs[L].px.n_valid <= total && recs[L].n_outliers <= recs[L].px.n_valid && recs[L].px.trials <= 6);
                    if (!strcmp(mk.name, "none")) CHECK(recs[L].px.n_valid0 == 0 && (recs[L].px.flags == pa::FEW_PIXELS || recs[L].px.flags == pa::DEGENERATE));
                }
                if (!strcmp(mk.name, "all")) {
                    photo_robust_ref::align(i1.data(), i2.data(), x0, o, 4, want);
                    CHECK(memcmp(recs, want, sizeof recs) == 0);
                }
            }

    // the right half of img1 is noise and the mask hides it: the records are those of the clean img1 under the same mask, bit for bit, and find the move
    {
        pr::Opts o;
        pr::default_opts(o);
        o.base.max_iterations = 24;
        pr::Record recs[pa::MAX_LEVELS], clean[pa::MAX_LEVELS];
        memset(recs, 0, sizeof recs);
        memset(clean, 0, sizeof clean);
        const std::vector<uint8_t>& left = masks[7].m;
        photo_masked_ref::align(spoiled.data(), left.data(), i2.data(), zero, o, 4, recs);
        photo_masked_ref::align(i1.data(), left.data(), i2.data(), zero, o, 4, clean);
        CHECK(memcmp(recs, clean, sizeof recs) == 0);
        double worst = 0.0;
        for (int k = 0; k < 8; k++) worst = std::fmax(worst, std::fabs((double)recs[0].px.offsets_px[k] - (k % 2 ? DY : DX)));
        printf("left half of a half-spoiled img1: %.4f px off, n_valid %d, flags %d\n", worst, recs[0].px.n_valid, recs[0].px.flags);
        CHECK(worst < 0.5 && recs[0].px.n_valid <= NPIX / 2);
    }
    // the localise rule (include/hnet_keyframe_localise.h) on hostile entries, masks, counts, records, states and options: every combination writes a whole
    // record with one known flag, and a call that is not LOCALISED with apply changes no byte of any state
    {
        namespace kl = hnet_localise;
        kl::km::Entry ent[8];
        memset(ent, 0, sizeof ent);
        for (int j = 0; j < 8; j++) {
            ent[j].valid = j != 2;
            ent[j].links = j == 5 ? 0x7fffffff : j;
            for (int k = 0; k < 9; k++) ent[j].h_origin_key[k] = j == 3 ? NAN : (j == 4 ? 0.0 : (k % 4 == 0 ? 1.0 : (k == 2 ? 1e6 * j : 0.0)));
        }
        pr::Record good, hostile[4];
        memset(&good, 0, sizeof good);
        good.px.n_valid = 60000;
        good.px.mse = 1.0;
        for (int i = 0; i < 4; i++) hostile[i] = good;
        hostile[1].px.offsets_px[3] = nanp[3];
        for (int k = 0; k < 8; k++) { hostile[2].px.offsets_px[k] = big; hostile[3].px.offsets_px[k] = line[k]; }
        hostile[0].px.flags = pa::SINGULAR;
        const double views[3][9] = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {1e300, 0, 0, 0, 1e300, 0, 0, 0, 1e300}, {0, 0, 0, 0, 0, 0, 0, 0, 0}};
        const int masks_[] = {0, 1, 0xff, -1, 0x100};
        const uint64_t counts[] = {0, 35840, 71680, ~(uint64_t)0};
        int seen = 0;
        for (int slot : {-1, 0, 7, 8, 1000, -5})
            for (int um : masks_)
                for (uint64_t nc : counts)
                    for (const auto& v : views)
                        for (int h = 0; h < 5; h++)
                            for (int ap = 0; ap < 2; ap++) {
                                kl::Opts o;
                                kl::default_opts(o);
                                o.apply = ap;
                                o.max_shift_px = h == 2 ? 1e-300 : 0.0;
                                kl::kf::State st, ns;
                                memset(&st, 0, sizeof st);
                                st.has_key = 1;
                                if (slot == 7) memcpy(st.key_px, line, 32);
                                kl::km::MapState m = {slot, slot == 1000 ? -3 : 9, 0, 4}, nm;
                                kl::km::Entry ne[8];
                                kl::Localise out;
                                memset(&out, 0xA5, sizeof out);
                                const pr::Record& rec = h < 4 ? hostile[h] : good;
                                out.rec = rec;
                                const int loc = kl::decide_localise(&st, &m, ent, 8, um, nc, v, out.rec, o, &ns, &nm, ne, out);
                                const int f = out.flags;
                                CHECK(f && !(f & (f - 1)) && f <= kl::LOC_LOCALISED && loc == (f == kl::LOC_LOCALISED) && out.pad[0] == 0 && out.pad[1] == 0);
                                if (!(loc && ap)) CHECK(memcmp(&ns, &st, sizeof st) == 0 && memcmp(&nm, &m, sizeof m) == 0 && memcmp(ne, ent, sizeof ent) == 0);
                                if (!loc) CHECK(memcmp(out.h_origin_curr, out.h_origin_before, 72) == 0 && out.links == out.links_before);
                                seen |= f;
                            }
        printf("localise rule: flags reached 0x%x\n", seen);
        CHECK(seen & kl::LOC_LOCALISED);
        CHECK(seen & kl::LOC_CHAIN);
    }
    if (failures) { printf("photo_masked_check: %d FAILED\n", failures); return 1; }
    printf("photo_masked_check: ok\n");
    return 0;
}
