// filters_photo_gate_ref.cpp — the host reference of the photometric gate of hnet_filters (include/hnet.h hnet_filters_set_photo_gate) as a small shared
// library for the tests: include/hnet_ekf.h's photo_reject / iterated_update_photo_gated behind a C interface on the hnet.h structs, fed the states after
// propagation, a step's network outputs and SCRIPTED photometric records (the header never looks at an image: its callable is handed 8 offsets and returns
// a record), with iterated_update_gated next to it in the same build (the bitwise comparisons of tests/test_filters_photo_gate_cpu.py).
// Build: g++ -std=c++17 -O2 -shared -fPIC -pthread -I include tests/cpp/filters_photo_gate_ref.cpp -o <lib>.so
#include "hnet.h"
#include "hnet_ekf.h"

#include <cstring>
#include <vector>

using hnet_ekf::Innovation;
using hnet_ekf::PhotoRecord;
using hnet_ekf::State;

static_assert(sizeof(hnet_filter_state) == sizeof(double) + sizeof(State), "hnet_filter_state = t + hnet_ekf::State");
static_assert(sizeof(hnet_photo_residual) == sizeof(PhotoRecord) && offsetof(hnet_photo_residual, n_inside) == offsetof(PhotoRecord, n_inside) &&
              offsetof(hnet_photo_residual, flags) == offsetof(PhotoRecord, flags), "hnet_photo_residual = hnet_ekf::PhotoRecord");
static_assert((int)HNET_PHOTO_DEGENERATE == (int)hnet_ekf::PHOTO_DEGENERATE && (int)HNET_PHOTO_REJECTED == (int)hnet_ekf::PHOTO_REJECTED, "HNET_PHOTO_* are the header's flags");

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

// the network surface of filters_innov_ref.cpp: record `it` of net72 [iters][72], the gate as latest time / image count; counts its calls
struct FakeNet {
    const float* net72;
    int gate;
    double t_frame;
    int img_counter;
    int calls = 0;
    int it = -1;                         // the iteration of the last call; -1 before the first
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
// the scripted photometric callable: before the first forward it is asked for the prior's record (script[0]), after forward `it` for that estimate's
// (script[1 + it]); it notes how often it was called and the offsets it was handed
struct ScriptedPhoto {
    const FakeNet* net;
    const hnet_photo_residual* script;
    int calls = 0;
    double* offsets = nullptr;           // [1 + iters][8] or null
    PhotoRecord operator()(const double* off_px) {
        const int k = net->it < 0 ? 0 : 1 + net->it;
        calls++;
        for (int i = 0; offsets && i < 8; i++) offsets[k * 8 + i] = off_px[i];
        return from_c(script[k]);
    }
};
}  // namespace

extern "C" {

int photo_gate_ref_reject(const hnet_photo_residual* prior, const hnet_photo_residual* est, double max_ratio, int min_inside) {
    return hnet_ekf::photo_reject(from_c(*prior), from_c(*est), max_ratio, min_inside) ? 1 : 0;
}

// hnet_ekf::iterated_update_photo_gated fed with net72 [iters][72] and the scripted records script [1 + iters] ([0]: of the prior, [1 + it]: of forward it's
// mean).  out [iters]; prec [1 + iters]: the header's records (zeros where it formed none).  Returns the updates applied, -1 - applied when a singular S
// ended the loop early.  calls / photo_calls: how often the network / the photometric callable ran; offsets [1 + iters][8]: what the callable was handed.
// The last three may be null.
int photo_gate_ref_iterated(hnet_filter_state* st, const hnet_filter_params* p, int iters, const float* net72, int gate, double max_nis,
                            const hnet_photo_residual* script, double max_ratio, int min_inside, hnet_innovation* out, hnet_photo_residual* prec, int* calls,
                            int* photo_calls, double* offsets) {
    State s = load(*st);
    FakeNet net{net72, gate, st->t, gate ? 11 : 0};
    ScriptedPhoto photo{&net, script};
    photo.offsets = offsets;
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
    if (photo_calls) *photo_calls = photo.calls;
    return singular ? -1 - done : done;
}

// hnet_ekf::iterated_update_gated in this build, with the same network
int photo_gate_ref_iterated_nis(hnet_filter_state* st, const hnet_filter_params* p, int iters, const float* net72, int gate, double max_nis, hnet_innovation* out,
                                int* calls) {
    State s = load(*st);
    FakeNet net{net72, gate, st->t, gate ? 11 : 0};
    double prior[8];
    std::vector<Innovation> rec(iters);
    const int done = hnet_ekf::iterated_update_gated(s, net, iters, p->k_net_cov, prior, st->t, max_nis, rec.data());
    save(s, *st);
    bool singular = false;
    for (int it = 0; it < iters; it++) {
        to_record(rec[it], it, out[it]);
        singular |= rec[it].flag == hnet_ekf::INNOV_SINGULAR;
    }
    if (calls) *calls = net.calls;
    return singular ? -1 - done : done;
}

}  // extern "C"
