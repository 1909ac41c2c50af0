// filters_photo_refine_ref.cpp — the host reference of the photometric fallback of hnet_filters (include/hnet.h hnet_filters_set_photo_refine)
// as a small shared library for the tests: include/hnet_photo_refine.h's marginal, refine_measurement and hnet_ekf::iterated_update_photo_refined behind
// a C interface on the hnet.h structs.  The loop is fed as tests/cpp/filters_photo_gate_ref.cpp feeds iterated_update_photo_gated (the states after
// propagation, a step's network outputs, SCRIPTED photometric records) and a STUB aligner that hands back a given level-0 record and accepted count
// (the header never looks at an image); iterated_update_photo_gated and update / reset_4pt_offset by hand stand next to it in the same build (the
// bitwise comparisons of tests/test_filters_photo_refine_cpu.py).
// Build: g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -pthread -I include tests/cpp/filters_photo_refine_ref.cpp -o <lib>.so
#include "hnet.h"
#include "hnet_photo_refine.h"

#include <cstring>
#include <vector>

using hnet_ekf::Innovation;
using hnet_ekf::PhotoRecord;
using hnet_ekf::State;

static_assert(sizeof(hnet_filter_state) == sizeof(double) + sizeof(State), "hnet_filter_state = t + hnet_ekf::State");
static_assert(sizeof(hnet_photo_residual) == sizeof(PhotoRecord), "hnet_photo_residual = hnet_ekf::PhotoRecord");
static_assert(sizeof(hnet_photo_robust) == sizeof(hnet_robust::Record) && offsetof(hnet_photo_robust, info10) == offsetof(hnet_robust::Record, info10),
              "hnet_photo_robust = hnet_robust::Record");
static_assert(sizeof(hnet_photo_refine) == sizeof(hnet_refine::Record) && offsetof(hnet_photo_refine, r_px) == offsetof(hnet_refine::Record, r_px) &&
              offsetof(hnet_photo_refine, innov) == offsetof(hnet_refine::Record, r) && offsetof(hnet_photo_refine, flags) == offsetof(hnet_refine::Record, flags),
              "hnet_photo_refine = hnet_refine::Record");
static_assert(sizeof(hnet_photo_refine_opts) == sizeof(hnet_refine::Opts) && offsetof(hnet_photo_refine_opts, cov_scale) == offsetof(hnet_refine::Opts, cov_scale) &&
              offsetof(hnet_photo_refine_opts, max_mse) == offsetof(hnet_refine::Opts, max_mse), "hnet_photo_refine_opts = hnet_refine::Opts");
static_assert((int)HNET_REFINE_ASKED == hnet_refine::ASKED && (int)HNET_REFINE_APPLIED == hnet_refine::APPLIED && (int)HNET_REFINE_NIS_REJECTED == hnet_refine::NIS_REJECTED &&
              (int)HNET_REFINE_S_SINGULAR == hnet_refine::S_SINGULAR && (int)HNET_REFINE_BAD_K_NET_COV == hnet_refine::BAD_K_NET_COV &&
              (int)HNET_REFINE_STOPPED == hnet_refine::STOPPED && (int)HNET_REFINE_NO_STEP == hnet_refine::NO_STEP && (int)HNET_REFINE_MSE_ABOVE_MAX == hnet_refine::MSE_ABOVE_MAX &&
              (int)HNET_REFINE_NO_FACTOR == hnet_refine::NO_FACTOR && (int)HNET_REFINE_NON_FINITE == hnet_refine::NON_FINITE && (int)HNET_REFINE_UNUSABLE == hnet_refine::UNUSABLE,
              "HNET_REFINE_* are the header's flags");

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
hnet_robust::Record robust(const hnet_photo_robust& r) { hnet_robust::Record o; std::memcpy(&o, &r, sizeof o); return o; }
hnet_refine::Opts refine_opts(const hnet_photo_refine_opts& r) { hnet_refine::Opts o; std::memcpy(&o, &r, sizeof o); return o; }

// the network surface and the scripted photometric callable of filters_photo_gate_ref.cpp
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
// the stub aligner: the given record and accepted count; notes its calls and the start it was handed
struct StubAlign {
    const hnet_photo_robust* rec;
    int accepted_total;
    int calls = 0;
    float x0[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    void operator()(const float* start, hnet_robust::Record& out, int& accepted) {
        calls++;
        std::memcpy(x0, start, sizeof x0);
        out = robust(*rec);
        accepted = accepted_total;
    }
};
}  // namespace

extern "C" {

int photo_refine_ref_opts_valid(const hnet_photo_refine_opts* o) { return hnet_refine::opts_valid(refine_opts(*o)) ? 1 : 0; }

int photo_refine_ref_marginal(const hnet_photo_robust* rec, double* info8, double* grad8) { return hnet_refine::marginal(robust(*rec), info8, grad8) ? 1 : 0; }

// -> 1 usable (out72, r_px written), 0 unusable (the reason bit or-ed into *flags, nothing else written)
int photo_refine_ref_measurement(const hnet_photo_robust* rec, int accepted_total, const hnet_photo_refine_opts* o, double k_net_cov, float* out72, double* r_px,
                                 int32_t* flags) {
    return hnet_refine::refine_measurement(robust(*rec), accepted_total, refine_opts(*o), k_net_cov, out72, r_px, *flags) ? 1 : 0;
}

// hnet_ekf::innovation of the packed measurement m72 on the state, with the state's own prior
int photo_refine_ref_innovation(const hnet_filter_state* st, const hnet_filter_params* p, const float* m72, hnet_innovation* out) {
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
int photo_refine_ref_update(hnet_filter_state* st, const hnet_filter_params* p, const float* m72, int update_offset, int reset) {
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

// hnet_ekf::iterated_update_photo_refined fed with net72 [iters][72], the scripted records script [1 + iters] and the stub aligner's record.  refine: null =
// refinement off.  out [iters], prec [1 + iters], rout: the header's records.  Returns the updates applied, -1 - applied when a singular S ended the loop or
// the fallback.  calls / align_calls: how often the network / the aligner ran; x0 [8]: the start the aligner was handed.  The last three may be null.
int photo_refine_ref_iterated(hnet_filter_state* st, const hnet_filter_params* p, int iters, const float* net72, int gate, double max_nis,
                              const hnet_photo_residual* script, double max_ratio, int min_inside, const hnet_photo_refine_opts* refine, const hnet_photo_robust* align_rec,
                              int accepted_total, hnet_innovation* out, hnet_photo_residual* prec, hnet_photo_refine* rout, int* calls, int* align_calls, float* x0) {
    State s = load(*st);
    FakeNet net{net72, gate, st->t, gate ? 11 : 0};
    ScriptedPhoto photo{&net, script};
    StubAlign align{align_rec, accepted_total};
    double prior[8];
    std::vector<Innovation> rec(iters);
    std::vector<PhotoRecord> pr(1 + iters);
    hnet_refine::Opts ro;
    if (refine) ro = refine_opts(*refine);
    hnet_refine::Record rr;
    const int done = hnet_ekf::iterated_update_photo_refined(s, net, iters, p->k_net_cov, prior, st->t, max_nis, rec.data(), photo, max_ratio, min_inside, pr.data(),
                                                             refine ? &ro : nullptr, align, rr);
    save(s, *st);
    bool singular = (rr.flags & hnet_refine::S_SINGULAR) != 0;
    for (int it = 0; it < iters; it++) {
        to_record(rec[it], it, out[it]);
        singular |= rec[it].flag == hnet_ekf::INNOV_SINGULAR;
    }
    for (int k = 0; k <= iters; k++) prec[k] = to_c(pr[k]);
    std::memcpy(rout, &rr, sizeof rr);
    if (calls) *calls = net.calls;
    if (align_calls) *align_calls = align.calls;
    if (x0) std::memcpy(x0, align.x0, sizeof align.x0);
    return singular ? -1 - done : done;
}

// hnet_ekf::iterated_update_photo_gated in this build, with the same network and script
int photo_refine_ref_iterated_gated(hnet_filter_state* st, const hnet_filter_params* p, int iters, const float* net72, int gate, double max_nis,
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
