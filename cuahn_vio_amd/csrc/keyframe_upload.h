// keyframe_upload.h — the ONE upload block of the operator-level keyframe calls (hnet_op_keyframe_render, _localise, _adjust, _adjust_solve): a map of m
// entries passed as one session, {id 0 padded to 8 bytes | [view 9 f64] | entries [m] | [seeded adjust record | [infos]] | [images [m]] | [frame]}.  The id,
// the view, the entries, the record and the infos lie at 8-byte boundaries (the device reads them as doubles), the images and the frame at 16-byte
// boundaries (it reads them as uint4).  No HIP here: tests/cpp/keyframe_upload_check.cpp compiles this header with g++ and pins every layout in use.
#pragma once
#include <cstddef>

namespace capi __attribute__((visibility("hidden"))) {

struct KeyUpload {
    enum : unsigned { VIEW = 1, SEED = 2, INFOS = 4, IMAGES = 8, FRAME = 16 };      // the optional sections (INFOS: only behind SEED)
    // the sections' sizes; keyframes_internal.h asserts them against the device's types
    static constexpr size_t VIEW_BYTES = 9 * sizeof(double), ENTRY_BYTES = 88, SEED_BYTES = 4288, INFOS_BYTES = 28 * 64 * sizeof(double), IMAGE_BYTES = 224 * 320;
    size_t view = 0, entry = 0, seed = 0, infos = 0, images = 0, frame = 0, total = 0;   // offsets (an absent section: where it would begin) and the block's size
    constexpr KeyUpload(int m, unsigned sections) {
        size_t at = 8;                         // behind the id and its padding
        view = at;
        if (sections & VIEW) at += VIEW_BYTES;
        entry = at;
        at += (size_t)m * ENTRY_BYTES;
        seed = at;
        if (sections & SEED) at += SEED_BYTES;
        infos = at;
        if (sections & INFOS) at += INFOS_BYTES;
        if (sections & (IMAGES | FRAME)) at = (at + 15) & ~(size_t)15;
        images = at;
        if (sections & IMAGES) at += (size_t)m * IMAGE_BYTES;
        frame = at;
        if (sections & FRAME) at += IMAGE_BYTES;
        total = at;
    }
};
static_assert(KeyUpload::ENTRY_BYTES % 8 == 0 && KeyUpload::SEED_BYTES % 8 == 0 && KeyUpload::IMAGE_BYTES % 16 == 0, "a section keeps the next one's alignment");

}  // namespace capi
