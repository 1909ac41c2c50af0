// filters_keyframe_ref.cpp — the host reference of the keyframe track as an in-step filter measurement (include/hnet.h hnet_filters_set_keyframe_measure;
// DESIGN 7v) as a small shared library for the tests: include/hnet_keyframe_measure.h's step, usability tests, z, measure and
// hnet_ekf::iterated_update_keyframe_measured behind a C interface on the hnet.h structs, on top of keyframe_ref.cpp (compose, decide and the host robust
// alignment).  The loop is fed as tests/cpp/filters_photo_refine_ref.cpp feeds iterated_update_photo_refined (the states after propagation, a step's network
// outputs, SCRIPTED photometric records) and either a STUB aligner that hands back a given level-0 record and accepted count, or the host robust alignment
// on a keyframe and a current frame; iterated_update_photo_gated and update / reset_4pt_offset by hand stand next to it in the same build (the bitwise
// comparisons of tests/test_filters_keyframe_cpu.py).
// Built as keyframe_ref.cpp is built (nothing may be contracted), with -I include.
#include "keyframe_ref.cpp"

#include "hnet.h"
#include "hnet_keyframe_measure.h"

#include <vector>

using hnet_ekf::Innovation;
using hnet_ekf::PhotoRecord;
using hnet_ekf::State;
namespace kfm = hnet_kfm;

static_assert(sizeof(hnet_filter_state) == sizeof(double) + sizeof(State), "hnet_filter_state = t + hnet_ekf::State");
static_assert(sizeof(hnet_photo_residual) == sizeof(PhotoRecord), "hnet_photo_residual = hnet_ekf::PhotoRecord");
static_assert(sizeof(hnet_keyframe_track) == sizeof(kf::Track) && sizeof(hnet_keyframe_opts) == sizeof(kf::Opts), "the track's layouts");
static_assert(sizeof(hnet_keyframe_measure) == sizeof(kfm::Record) && offsetof(hnet_keyframe_measure, step_px) == offsetof(kfm::Record, step_px) &&
              offsetof(hnet_keyframe_measure, z_px) == offsetof(kfm::Record, z_px) && offsetof(hnet_keyframe_measure, r_px) == offsetof(kfm::Record, r_px) &&
              offsetof(hnet_keyframe_measure, innov) == offsetof(kfm::Record, r) && offsetof(hnet_keyframe_measure, flags) == offsetof(kfm::Record, flags),
              "hnet_keyframe_measure = hnet_kfm::Record");
static_assert(sizeof(hnet_keyframe_measure_opts) == sizeof(kfm::Opts) && offsetof(hnet_keyframe_measure_opts, cov_scale) == offsetof(kfm::Opts, cov_scale) &&
              offsetof(hnet_keyframe_measure_opts, when) == offsetof(kfm::Opts, when), "hnet_keyframe_measure_opts = hnet_kfm::Opts");
static_assert(sizeof(kfm::Session) == 128, "the session the tests carry: the keyframe state (120 bytes), prev_ok, pad");

namespace {
State load(const hnet_filter_state& r) { State s; std::memcpy(&s, &r.p[0], sizeof s); return s; }
void save(const State& s, hnet_filter_state& r) { std::memcpy(&r.p[0], &s, sizeof s); }
void to_record(const Innovation& a, int it, hnet_innovation& o) {
    std::memcpy(o.r, a.r, sizeof o.r);
    std::memcpy(o.s_diag, a.s_diag, sizeof o.s_diag);
    o.nis = a.nis;
    o.iteration = it;
    o.flag = a.flag;
}
PhotoRecord from_c(const hnet_photo_residual& r) { return PhotoRecord{r.sum, r.sum_inside, r.n_inside, r.flags}; }
hnet_photo_residual to_c(const PhotoRecord& r) { return hnet_photo_residual{r.sum, r.sum_inside, r.n_inside, r.flags}; }
kfm::Opts measure_opts(const hnet_keyframe_measure_opts& r) { kfm::Opts o; std::memcpy(&o, &r, sizeof o); return o; }

// the network surface and the scripted photometric callable of filters_photo_refine_ref.cpp
struct FakeNet {
    const float* net72;
    int gate;
    double t_frame;
    int img_counter;
    int calls = 0;
    int it = -1;
    const float* cur = nullptr;
    struct M { const float* v; double operator()(int i, int j) const { return v[i * 8 + j]; } };
    struct V { const float* v; double operator()(int i, int) const { return v[i]; } };
    template <class P> void network_inference(const P&, int iteration) {
        cur = net72 + (size_t)iteration * 72;
        it = iteration;
        calls++;
    }
    double get_latest_inference_time() const { return gate ? t_frame : t_frame - 1.0; }
    V get_pred_mean() const { return V{cur}; }
    M get_pred_Cov() const { return M{cur + 8}; }
};
struct ScriptedPhoto {
    const FakeNet* net;
    const hnet_photo_residual* script;
    PhotoRecord operator()(const double*) { return from_c(script[net->it < 0 ? 0 : 1 + net->it]); }
};
// the aligner: the host robust alignment keyframe -> curr when there are frames, else the stub's record and accepted count; notes its calls and its start
struct Aligner {
    const uint8_t *keyframe, *curr;
    const hnet_robust::Opts* align;
    int levels;
    const hnet_photo_robust* stub;
    int stub_accepted;
    int calls = 0;
    float x0[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    void operator()(const float* start, hnet_robust::Record& out, int& accepted) {
        calls++;
        std::memcpy(x0, start, sizeof x0);
        if (keyframe) {
            hnet_robust::Record recs[hnet_align::MAX_LEVELS];
            std::memset(recs, 0, sizeof recs);
            photo_robust_ref::align(keyframe, curr, start, *align, levels, recs);
            out = recs[0];
            accepted = 0;
            for (int l = 0; l < levels; l++) accepted += recs[l].px.accepted;
        } else {
            std::memcpy(&out, stub, sizeof out);
            accepted = stub_accepted;
        }
    }
};
}  // namespace

extern "C" {

void filters_keyframe_ref_default_opts(hnet_keyframe_measure_opts* o) {
    kfm::Opts d;
    kfm::default_opts(d);
    std::memcpy(o, &d, sizeof d);
}
int filters_keyframe_ref_opts_valid(const hnet_keyframe_measure_opts* o) { return kfm::opts_valid(measure_opts(*o)) ? 1 : 0; }

// step_px [8] of a state
void filters_keyframe_ref_step(const hnet_filter_state* st, float* step_px) {
    const State s = load(*st);
    for (int k = 0; k < 8; k++) step_px[k] = kfm::step_entry(s, k);
}

// 1 and z_px [8] written, or 0
int filters_keyframe_ref_relative_z(const float* key_px_prev, const float* key_px_curr, float* z_px) { return kfm::relative_z(key_px_prev, key_px_curr, z_px) ? 1 : 0; }

// -> 1 usable (z_px, r_px, out72 written), 0 unusable (the reason bit or-ed into *flags, nothing else written)
int filters_keyframe_ref_measure(int had_key, const float* key_px_prev, int prev_ok, const hnet_keyframe_track* track, int accepted_total,
                                 const hnet_keyframe_measure_opts* o, double k_net_cov, float* z_px, double* r_px, float* out72, int32_t* flags) {
    kf::Track t;
    std::memcpy(&t, track, sizeof t);
    return kfm::measure(had_key != 0, key_px_prev, prev_ok, t, accepted_total, measure_opts(*o), k_net_cov, z_px, r_px, out72, *flags) ? 1 : 0;
}

int filters_keyframe_ref_selected(int when, int updates) { return kfm::selected(when, updates) ? 1 : 0; }

// hnet_ekf::innovation of the packed measurement m72 on the state, with the state's own prior
int filters_keyframe_ref_innovation(const hnet_filter_state* st, const hnet_filter_params* p, const float* m72, hnet_innovation* out) {
    const State s = load(*st);
    double prior_px[8], prior_cam[8], mean[8], cov[64];
    hnet_ekf::prior_pixels(s, prior_px, prior_cam);
    for (int i = 0; i < 8; i++) mean[i] = (double)m72[i];
    for (int e = 0; e < 64; e++) cov[e] = (double)m72[8 + e];
    Innovation a;
    const bool ok = hnet_ekf::innovation(s, mean, cov, prior_cam, p->k_net_cov, a);
    to_record(a, 0, *out);
    return ok ? 1 : 0;
}

// by hand: update with the packed measurement against the state's own prior (update_offset as given), then reset_4pt_offset when `reset`
int filters_keyframe_ref_update(hnet_filter_state* st, const hnet_filter_params* p, const float* m72, int update_offset, int reset) {
    State s = load(*st);
    double prior_px[8], prior_cam[8], mean[8], cov[64];
    hnet_ekf::prior_pixels(s, prior_px, prior_cam);
    for (int i = 0; i < 8; i++) mean[i] = (double)m72[i];
    for (int e = 0; e < 64; e++) cov[e] = (double)m72[8 + e];
    const bool ok = hnet_ekf::update(s, mean, cov, prior_cam, p->k_net_cov, update_offset != 0);
    if (reset) hnet_ekf::reset_4pt_offset(s);
    save(s, *st);
    return ok ? 1 : 0;
}
void filters_keyframe_ref_reset(hnet_filter_state* st) {
    State s = load(*st);
    hnet_ekf::reset_4pt_offset(s);
    save(s, *st);
}

// hnet_ekf::iterated_update_keyframe_measured fed with net72 [iters][72] and the scripted records script [1 + iters].  measure: null = the feature off.
// session [128 bytes]: hnet_kfm::Session, read and advanced.  keyframe / curr: the frames [71 680] the host robust alignment runs on (a copy flag copies
// curr into keyframe), or keyframe null: the stub record align_rec and accepted_total.  out [iters], prec [1 + iters], rout: the header's records.
// Returns the updates applied, -1 - applied when a singular S ended the loop or the keyframe update.  calls / align_calls: how often the network / the
// aligner ran; x0 [8]: the start the aligner was handed; copy: decide's copy flag.  The last four may be null.
int filters_keyframe_ref_iterated(hnet_filter_state* st, const hnet_filter_params* p, int iters, const float* net72, int gate, double max_nis,
                                  const hnet_photo_residual* script, double max_ratio, int min_inside, const hnet_keyframe_measure_opts* measure, int gap,
                                  void* session, uint8_t* keyframe, const uint8_t* curr, const hnet_photo_robust* align_rec, int accepted_total,
                                  hnet_innovation* out, hnet_photo_residual* prec, hnet_keyframe_measure* rout, int* calls, int* align_calls, float* x0, int* copy) {
    State s = load(*st);
    FakeNet net{net72, gate, st->t, gate ? 11 : 0};
    ScriptedPhoto photo{&net, script};
    kfm::Opts mo;
    if (measure) mo = measure_opts(*measure);
    else kfm::default_opts(mo);
    Aligner align{keyframe, curr, &mo.track.align, mo.track.levels, align_rec, accepted_total};
    kfm::Session ks;
    std::memcpy(&ks, session, sizeof ks);
    double prior[8];
    std::vector<Innovation> rec(iters);
    std::vector<PhotoRecord> pr(1 + iters);
    kfm::Record rr;
    int cp = 0;
    const int done = hnet_ekf::iterated_update_keyframe_measured(s, net, iters, p->k_net_cov, prior, st->t, max_nis, rec.data(), photo, max_ratio, min_inside, pr.data(),
                                                                 measure ? &mo : nullptr, gap != 0, ks, align, rr, &cp);
    save(s, *st);
    std::memcpy(session, &ks, sizeof ks);
    if (cp && keyframe) std::memcpy(keyframe, curr, photo_ref::NPIX);
    bool singular = (rr.flags & kfm::S_SINGULAR) != 0;
    for (int it = 0; it < iters; it++) {
        to_record(rec[it], it, out[it]);
        singular |= rec[it].flag == hnet_ekf::INNOV_SINGULAR;
    }
    for (int k = 0; k <= iters; k++) prec[k] = to_c(pr[k]);
    std::memcpy(rout, &rr, sizeof rr);
    if (calls) *calls = net.calls;
    if (align_calls) *align_calls = align.calls;
    if (x0) std::memcpy(x0, align.x0, sizeof align.x0);
    if (copy) *copy = cp;
    return singular ? -1 - done : done;
}

// hnet_ekf::iterated_update_photo_gated in this build, with the same network and script
int filters_keyframe_ref_iterated_gated(hnet_filter_state* st, const hnet_filter_params* p, int iters, const float* net72, int gate, double max_nis,
                                        const hnet_photo_residual* script, double max_ratio, int min_inside, hnet_innovation* out, hnet_photo_residual* prec, int* calls) {
    State s = load(*st);
    FakeNet net{net72, gate, st->t, gate ? 11 : 0};
    ScriptedPhoto photo{&net, script};
    double prior[8];
    std::vector<Innovation> rec(iters);
    std::vector<PhotoRecord> pr(1 + iters);
    const int done = hnet_ekf::iterated_update_photo_gated(s, net, iters, p->k_net_cov, prior, st->t, max_nis, rec.data(), photo, max_ratio, min_inside, pr.data());
    save(s, *st);
    bool singular = false;
    for (int it = 0; it < iters; it++) {
        to_record(rec[it], it, out[it]);
        singular |= rec[it].flag == hnet_ekf::INNOV_SINGULAR;
    }
    for (int k = 0; k <= iters; k++) prec[k] = to_c(pr[k]);
    if (calls) *calls = net.calls;
    return singular ? -1 - done : done;
}

}  // extern "C"
