// keyframe_localise_ref.cpp — the rule of include/hnet_keyframe_localise.h behind a C interface (include/hnet.h hnet_op_keyframe_localise):
// the header's own functions, called one at a time by tests/keyframe_localise_util.py.  The template of a localise is keyframe_render_ref.cpp's render and its
// alignment photo_masked_ref.cpp's; this file adds only the rule.  Built as those files are built:
//   g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -D__HIP_PLATFORM_AMD__ -I <rocm>/include -I cuahn_vio_amd/csrc -I include tests/cpp/keyframe_localise_ref.cpp
#include "photo_masked_ref.cpp"

#include "hnet_keyframe_localise.h"

namespace kl = hnet_localise;

extern "C" {

void keyframe_localise_ref_default_opts(void* o) { kl::default_opts(*static_cast<kl::Opts*>(o)); }
int keyframe_localise_ref_opts_valid(const void* o) { return kl::opts_valid(*static_cast<const kl::Opts*>(o)) ? 1 : 0; }

// mstate may be null (the operator-level call)
int keyframe_localise_ref_eligible_mask(const void* mstate, const void* entries, int capacity) {
    static_assert(sizeof(kl::Opts) == 104 && sizeof(kl::Localise) == 1808 && offsetof(kl::Localise, h_origin_before) == 1560 && offsetof(kl::Localise, used_mask) == 1784,
                  "the layouts of include/hnet.h");
    return kl::eligible_mask(static_cast<const kl::km::MapState*>(mstate), static_cast<const kl::km::Entry*>(entries), capacity);
}

void keyframe_localise_ref_start(int used_mask, uint64_t n_covered, const void* opts, float* x0) {
    kl::start(used_mask, n_covered, *static_cast<const kl::Opts*>(opts), x0);
}

// state / mstate null together: the operator-level call.  new_* receive the states after the call (may be null); out: the whole record, out.rec = *rec
int keyframe_localise_ref_decide(const void* state, const void* mstate, const void* entries, int capacity, int used_mask, uint64_t n_covered, const double* h_before,
                                 const void* rec, const void* opts, void* new_state, void* new_mstate, void* new_entries, void* out) {
    kl::Localise& r = *static_cast<kl::Localise*>(out);
    r.rec = *static_cast<const hnet_robust::Record*>(rec);
    return kl::decide_localise(static_cast<const kl::kf::State*>(state), static_cast<const kl::km::MapState*>(mstate), static_cast<const kl::km::Entry*>(entries),
                               capacity, used_mask, n_covered, h_before, r.rec, *static_cast<const kl::Opts*>(opts), static_cast<kl::kf::State*>(new_state),
                               static_cast<kl::km::MapState*>(new_mstate), static_cast<kl::km::Entry*>(new_entries), r);
}

}  // extern "C"
