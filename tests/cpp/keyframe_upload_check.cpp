// keyframe_upload_check.cpp — the upload block of the operator-level keyframe calls (cuahn_vio_amd/csrc/keyframe_upload.h) on the host, under
// AddressSanitizer + UBSan (tests/test_keyframe_upload_cpu.py): for every m in 1 .. 8 and every combination of the optional sections the offsets are
// aligned as the header promises, the sections present neither overlap nor leave the block, and the combinations the four calls use have the offsets
// the calls computed by hand before the header existed, written out here per m.  A block of `total` bytes is filled section by section, so that a
// section outside it is the sanitizer's finding too.
#include "../../cuahn_vio_amd/csrc/keyframe_upload.h"

#include <cstdio>
#include <cstring>
#include <vector>

using capi::KeyUpload;

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::printf("FAILED line %d (m %d, sections %#x): %s\n", __LINE__, m, s, #cond); \
            failures++;                                                              \
        }                                                                            \
    } while (0)

// the layouts of hnet_op_keyframe_render, _localise, _adjust and _adjust_solve as those calls wrote them: 88-byte entries, a 4288-byte record, 14336
// bytes of information matrices, 71680-byte images
static const size_t RENDER_IMG[8] = {176, 256, 352, 432, 528, 608, 704, 784};        // (80 + 88 m) rounded up to 16: view at 8, entries at 80
static const size_t ADJUST_IMG[8] = {96, 192, 272, 368, 448, 544, 624, 720};         // (8 + 88 m) rounded up to 16: entries at 8
static const size_t SOLVE_REC[8] = {96, 184, 272, 360, 448, 536, 624, 712};          // 8 + 88 m
static const size_t SOLVE_INFO[8] = {4384, 4472, 4560, 4648, 4736, 4824, 4912, 5000};        // + 4288

int main() {
    static_assert(KeyUpload::VIEW_BYTES == 72 && KeyUpload::ENTRY_BYTES == 88 && KeyUpload::SEED_BYTES == 4288 && KeyUpload::INFOS_BYTES == 14336 &&
                  KeyUpload::IMAGE_BYTES == 71680, "the sizes the literals above were worked out with");
    int combos = 0;
    for (int m = 1; m <= 8; m++)
        for (unsigned s = 0; s < 32; s++) {
            if ((s & KeyUpload::INFOS) && !(s & KeyUpload::SEED)) continue;      // (the infos belong to a seeded record)
            combos++;
            const KeyUpload u(m, s);
            struct Sec { size_t off, bytes, align; bool on; };
            const Sec sec[7] = {{0, 4, 8, true},                                // the id; its padding reaches to 8
                                {u.view, KeyUpload::VIEW_BYTES, 8, (s & KeyUpload::VIEW) != 0},
                                {u.entry, (size_t)m * KeyUpload::ENTRY_BYTES, 8, true},
                                {u.seed, KeyUpload::SEED_BYTES, 8, (s & KeyUpload::SEED) != 0},
                                {u.infos, KeyUpload::INFOS_BYTES, 8, (s & KeyUpload::INFOS) != 0},
                                {u.images, (size_t)m * KeyUpload::IMAGE_BYTES, 16, (s & KeyUpload::IMAGES) != 0},
                                {u.frame, KeyUpload::IMAGE_BYTES, 16, (s & KeyUpload::FRAME) != 0}};
            std::vector<unsigned char> block(u.total, 0);
            size_t end = 0;
            for (int i = 0; i < 7; i++) {
                if (!sec[i].on) continue;
                CHECK(sec[i].off % sec[i].align == 0);
                CHECK(sec[i].off >= end);                                        // in order, so no two overlap
                CHECK(sec[i].off + sec[i].bytes <= u.total);
                if (sec[i].off + sec[i].bytes > u.total) continue;
                for (size_t b = 0; b < sec[i].bytes; b++) CHECK(block[sec[i].off + b]++ == 0);
                end = sec[i].off + sec[i].bytes;
            }
            CHECK(end == u.total);                                               // nothing behind the last section
            CHECK(u.view == 8);
            const int k = m - 1;
            if (s == (KeyUpload::VIEW | KeyUpload::IMAGES)) {                   // hnet_op_keyframe_render
                CHECK(u.entry == 80 && u.images == RENDER_IMG[k] && u.total == RENDER_IMG[k] + (size_t)m * 71680);
            } else if (s == (KeyUpload::VIEW | KeyUpload::IMAGES | KeyUpload::FRAME)) {      // hnet_op_keyframe_localise
                CHECK(u.entry == 80 && u.images == RENDER_IMG[k] && u.frame == RENDER_IMG[k] + (size_t)m * 71680 && u.total == u.frame + 71680);
            } else if (s == KeyUpload::IMAGES) {                                 // hnet_op_keyframe_adjust
                CHECK(u.entry == 8 && u.images == ADJUST_IMG[k] && u.total == ADJUST_IMG[k] + (size_t)m * 71680);
            } else if (s == KeyUpload::SEED) {                                   // hnet_op_keyframe_adjust_solve without information matrices
                CHECK(u.entry == 8 && u.seed == SOLVE_REC[k] && u.infos == SOLVE_INFO[k] && u.total == SOLVE_INFO[k]);
            } else if (s == (KeyUpload::SEED | KeyUpload::INFOS)) {              // ... and with them
                CHECK(u.entry == 8 && u.seed == SOLVE_REC[k] && u.infos == SOLVE_INFO[k] && u.total == SOLVE_INFO[k] + 14336);
            }
        }
    if (combos != 8 * 24) {
        std::printf("FAILED: %d combinations walked, 192 expected\n", combos);
        failures++;
    }
    if (failures) return 1;
    std::printf("keyframe_upload_check: ok (%d layouts)\n", combos);
    return 0;
}
