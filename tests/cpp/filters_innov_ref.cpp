// filters_innov_ref.cpp — the host reference of the innovation records and the NIS gate of hnet_filters (include/hnet.h) as a small shared library for the
// tests and tools/filters_bench.py: include/hnet_ekf.h's innovation / iterated_update_gated behind a C interface on the hnet.h structs, fed the states
// after propagation and a step's network outputs, with iterated_update next to them in the same build (the bitwise comparisons of
// tests/test_filters_innov_cpu.py).  Build: g++ -std=c++17 -O2 -shared -fPIC -pthread -I include tests/cpp/filters_innov_ref.cpp -o <lib>.so
// With -DINNOV_REF_MAIN it is a program: it reads {int32 K, int32 iters} and K times {hnet_filter_state, hnet_filter_params, float net72[iters][72],
// int32 gate, double max_nis} from the file named on its command line and prints every record and the final states.
#include "hnet.h"
#include "hnet_ekf.h"

#include <cstdio>
#include <cstring>
#include <vector>

using hnet_ekf::Innovation;
using hnet_ekf::State;

static_assert(sizeof(hnet_filter_state) == sizeof(double) + sizeof(State), "hnet_filter_state = t + hnet_ekf::State");
static_assert(offsetof(hnet_innovation, iteration) == offsetof(Innovation, flag), "hnet_innovation = hnet_ekf::Innovation's doubles, then iteration and flag");
static_assert((int)HNET_INNOV_NONE == (int)hnet_ekf::INNOV_NONE && (int)HNET_INNOV_USED == (int)hnet_ekf::INNOV_USED && (int)HNET_INNOV_REJECTED == (int)hnet_ekf::INNOV_REJECTED &&
              (int)HNET_INNOV_SINGULAR == (int)hnet_ekf::INNOV_SINGULAR && (int)HNET_INNOV_SKIPPED == (int)hnet_ekf::INNOV_SKIPPED, "HNET_INNOV_* are the header's flags");

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

// the network surface iterated_update[_gated] drives: record `it` of net72 [iters][72], the gate as latest time / image count; counts its calls
struct FakeNet {
    const float* net72;
    int gate;
    double t_frame;
    int img_counter;
    int calls = 0;
    double* priors = nullptr;            // [iters][8] or null: the pixel prior every call was handed
    const float* cur = nullptr;
    struct M { const float* v; double operator()(int i, int j) const { return v[i * 8 + j]; } };
    struct V { const float* v; double operator()(int i, int) const { return v[i]; } };
    template <class P> void network_inference(const P& prior, int it) {
        cur = net72 + (size_t)it * 72;
        calls++;
        for (int i = 0; priors && i < 8; i++) priors[it * 8 + i] = prior[i];
    }
    double get_latest_inference_time() const { return gate ? t_frame : t_frame - 1.0; }
    V get_pred_mean() const { return V{cur}; }
    M get_pred_Cov() const { return M{cur + 8}; }
};
}  // namespace

extern "C" {

// hnet_ekf::innovation of `st` with a measurement given in doubles; returns 1, or 0 for a singular S.  out->iteration is set to 0.
int innov_ref_innovation(const hnet_filter_state* st, const double* mean_px, const double* cov_px, const double* prior_cam, double k_net_cov,
                         hnet_innovation* out) {
    const State s = load(*st);
    Innovation a;
    const bool ok = hnet_ekf::innovation(s, mean_px, cov_px, prior_cam, k_net_cov, a);
    to_record(a, 0, *out);
    return ok ? 1 : 0;
}

// hnet_ekf::iterated_update_gated fed with net72 [iters][72]; gate: the network's latest time is the frame's and it has seen > 10 images.  out [iters].
// Returns the updates applied, -1 - applied when a singular S ended the loop early (the convention of hnet_filters_step's updates); calls: how
// often the network ran; priors [iters][8]: the pixel prior of every call it made (what a host loop hands its forward; the prior of call `it` depends on
// records 0 .. it - 1 of net72 only).  Both may be null.
int innov_ref_iterated_gated(hnet_filter_state* st, const hnet_filter_params* p, int iters, const float* net72, int gate, double max_nis,
                             hnet_innovation* out, int* calls, double* priors) {
    State s = load(*st);
    FakeNet net{net72, gate, st->t, gate ? 11 : 0};
    net.priors = priors;
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

// hnet_ekf::iterated_update in this build, with the same network; returns its own return value
int innov_ref_iterated_plain(hnet_filter_state* st, const hnet_filter_params* p, int iters, const float* net72, int gate, int* calls) {
    State s = load(*st);
    FakeNet net{net72, gate, st->t, gate ? 11 : 0};
    double prior[8];
    const int done = hnet_ekf::iterated_update(s, net, iters, p->k_net_cov, prior, st->t);
    save(s, *st);
    if (calls) *calls = net.calls;
    return done;
}

// K sessions of a step: st [K] (after propagation), p [K], net72 [iters][K][72] as hnet_filters_step returns it, gate [K], max_nis [K]; out [iters][K],
// updates [K]; priors [iters][K][8] (may be null): the pixel prior each session's network call `it` was handed.  commit = 0 leaves st untouched: a host
// loop calls this once per iteration for the priors of its next batched forward (they depend on the earlier outputs only), then once more to commit.
void innov_ref_step(hnet_filter_state* st, const hnet_filter_params* p, int K, int iters, const float* net72, const int32_t* gate, const double* max_nis,
                    hnet_innovation* out, int32_t* updates, double* priors, int commit) {
    std::vector<float> one((size_t)iters * 72);
    std::vector<hnet_innovation> rec(iters);
    std::vector<double> pri((size_t)iters * 8);
    for (int k = 0; k < K; k++) {
        for (int it = 0; it < iters; it++) std::memcpy(&one[(size_t)it * 72], net72 + ((size_t)it * K + k) * 72, 72 * sizeof(float));
        hnet_filter_state w = st[k];
        updates[k] = innov_ref_iterated_gated(&w, p + k, iters, one.data(), gate[k], max_nis[k], rec.data(), nullptr, pri.data());
        if (commit) st[k] = w;
        for (int it = 0; it < iters; it++) {
            out[(size_t)it * K + k] = rec[it];
            if (priors) std::memcpy(priors + ((size_t)it * K + k) * 8, &pri[(size_t)it * 8], 8 * sizeof(double));
        }
    }
}

}  // extern "C"

#ifdef INNOV_REF_MAIN
int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s <input file>\n", argv[0]); return 2; }
    std::FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) { std::perror(argv[1]); return 2; }
    int32_t hdr[2];
    if (std::fread(hdr, sizeof hdr, 1, fp) != 1 || hdr[0] < 1 || hdr[0] > 65536 || hdr[1] < 1 || hdr[1] > 64) { std::fclose(fp); return 3; }
    const int K = hdr[0], iters = hdr[1];
    std::vector<float> net((size_t)iters * 72);
    std::vector<hnet_innovation> rec(iters);
    for (int k = 0; k < K; k++) {
        hnet_filter_state st;
        hnet_filter_params p;
        int32_t gate;
        double max_nis;
        if (std::fread(&st, sizeof st, 1, fp) != 1 || std::fread(&p, sizeof p, 1, fp) != 1 || std::fread(net.data(), sizeof(float), net.size(), fp) != net.size() ||
            std::fread(&gate, sizeof gate, 1, fp) != 1 || std::fread(&max_nis, sizeof max_nis, 1, fp) != 1) { std::fclose(fp); return 3; }
        const int upd = innov_ref_iterated_gated(&st, &p, iters, net.data(), gate, max_nis, rec.data(), nullptr, nullptr);
        std::printf("session %d updates %d\n", k, upd);
        for (int it = 0; it < iters; it++) {
            std::printf("  iteration %d flag %d nis %.17g\n    r     ", rec[it].iteration, rec[it].flag, rec[it].nis);
            for (int i = 0; i < 8; i++) std::printf(" %.17g", rec[it].r[i]);
            std::printf("\n    s_diag");
            for (int i = 0; i < 8; i++) std::printf(" %.17g", rec[it].s_diag[i]);
            std::printf("\n");
        }
        std::printf("  state");
        const double* d = &st.t;
        for (int i = 0; i < 29; i++) std::printf(" %.17g", d[i]);
        std::printf("\n  cov diagonal");
        for (int i = 0; i < 27; i++) std::printf(" %.17g", st.cov[i * 27 + i]);
        std::printf("\n");
    }
    std::fclose(fp);
    return 0;
}
#endif
