// keyframe_adjust_ref.cpp — the host reference of the joint adjustment of a keyframe map (include/hnet.h hnet_op_keyframe_adjust_solve,
// hnet_op_keyframe_adjust, hnet_sessions_keyframe_adjust): pairs, judge_edge, build, solve and finish of include/hnet_keyframe_adjust.h, the
// very functions the device compiles, under the header's Serial executor, around keyframe_map_ref.cpp's map and photo_robust_ref.cpp's alignment; one
// session's whole adjustment on the host.  Built as keyframe_map_ref.cpp is built (nothing may be contracted):
//   g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -D__HIP_PLATFORM_AMD__ -I <rocm>/include -I cuahn_vio_amd/csrc -I include tests/cpp/keyframe_adjust_ref.cpp
// With -DKEYFRAME_ADJUST_REF_MAIN (and without -shared) it is a stand-alone program that runs the header once over hostile inputs, for a sanitizer build.
#include "keyframe_map_ref.cpp"

#include <memory>

#include "hnet_keyframe_adjust.h"

namespace ka = hnet_adjust;

static_assert(sizeof(ka::Opts) == 136 && sizeof(ka::Job) == 48 && sizeof(ka::JobTable) == 8 + 28 * 48 && sizeof(ka::Edge) == 112 &&
              sizeof(ka::Record) == 40 + 24 + 512 + 576 + 28 * 112, "the layouts of include/hnet.h and csrc/keyframe_adjust_dev.h");

namespace {

// rec <- a zero record with the n rows of `edges`
void seed(ka::Record& rec, int n_edges, const ka::Edge* edges) {
    ka::record_zero(rec);
    rec.n_jobs = n_edges < 0 ? 0 : n_edges > ka::MAX_PAIRS ? ka::MAX_PAIRS : n_edges;
    for (int q = 0; q < rec.n_jobs; q++) rec.edge[q] = edges[q];
}

}  // namespace

extern "C" {

int keyframe_adjust_ref_pair_slots(int p, int m, int* i, int* j) { return ka::pair_slots(p, m, *i, *j) ? 1 : 0; }

// the job table of entries [m], every byte written
void keyframe_adjust_ref_pairs(const void* entries, int m, int min_grid, void* table) {
    ka::pairs(static_cast<const km::Entry*>(entries), m, min_grid, *static_cast<ka::JobTable*>(table));
}

void keyframe_adjust_ref_judge(const void* job, const void* rec, const void* opts, void* edge) {
    ka::judge_edge(*static_cast<const ka::Job*>(job), *static_cast<const hnet_robust::Record*>(rec), *static_cast<const ka::Opts*>(opts),
                   *static_cast<ka::Edge*>(edge));
}

int keyframe_adjust_ref_homography_d(const double* d, double* h) { return ka::homography_d(d, h) ? 1 : 0; }

// one edge's residual and one column of its Jacobian, as the solve calls them: G [9], di, dj, z, r and col [8]; which 0: endpoint i, 1: endpoint j
int keyframe_adjust_ref_edge_residual(const double* G, const double* di, const double* dj, const double* z, double* r) {
    return ka::edge_residual(G, di, dj, z, r) ? 1 : 0;
}
void keyframe_adjust_ref_jacobian_col(const double* G, const double* di, const double* dj, int which, int comp, double* col) {
    ka::jacobian_col(G, di, dj, which, comp, col);
}

// the solve alone: entries [m] (rewritten with apply), edges [n_edges], infos null or [n_edges][64] -> the record, every byte written
void keyframe_adjust_ref_solve(void* entries, int m, int n_edges, const void* edges, const double* infos, const void* opts, void* record) {
    ka::Record& rec = *static_cast<ka::Record*>(record);
    std::unique_ptr<ka::Problem> P(new ka::Problem);
    seed(rec, n_edges, static_cast<const ka::Edge*>(edges));
    ka::adjust_host(static_cast<km::Entry*>(entries), m, infos, *static_cast<const ka::Opts*>(opts), rec, *P);
}

// the header on alignment records that somebody else made: recs [the table's count], in job order.  This is what the device's full call is compared
// with, byte for byte, on ITS records (the host's own alignment sums in another order).
void keyframe_adjust_ref_adjust_with(void* entries, int m, const void* recs, const void* opts, void* record) {
    km::Entry* e = static_cast<km::Entry*>(entries);
    const ka::Opts& o = *static_cast<const ka::Opts*>(opts);
    const hnet_robust::Record* r = static_cast<const hnet_robust::Record*>(recs);
    ka::Record& rec = *static_cast<ka::Record*>(record);
    std::unique_ptr<ka::Problem> P(new ka::Problem);
    std::unique_ptr<double[]> infos(new double[ka::MAX_PAIRS * 64]);
    ka::JobTable t;
    ka::pairs(e, m, o.min_grid, t);
    ka::record_zero(rec);
    rec.n_jobs = t.count;
    for (int q = 0; q < t.count; q++) {
        ka::judge_edge(t.job[q], r[q], o, rec.edge[q]);
        for (int k = 0; k < 64; k++) infos[q * 64 + k] = r[q].px.info[k];
    }
    ka::adjust_host(e, m, infos.get(), o, rec, *P);
}

// the whole adjustment of m entries with images [m][71 680] on the host; edge_recs null or [28] level-0 records in job order (unused rows zero)
void keyframe_adjust_ref_adjust(void* entries, int m, const uint8_t* images, const void* opts, void* record, void* edge_recs) {
    const km::Entry* e = static_cast<const km::Entry*>(entries);
    const ka::Opts& o = *static_cast<const ka::Opts*>(opts);
    std::unique_ptr<hnet_robust::Record[]> r(new hnet_robust::Record[ka::MAX_PAIRS]);
    hnet_robust::Record recs[hnet_align::MAX_LEVELS];
    ka::JobTable t;
    memset(r.get(), 0, sizeof(hnet_robust::Record) * ka::MAX_PAIRS);
    ka::pairs(e, m, o.min_grid, t);
    for (int q = 0; q < t.count; q++) {
        memset(recs, 0, sizeof recs);
        photo_robust_ref::align(images + (size_t)t.job[q].i * photo_ref::NPIX, images + (size_t)t.job[q].j * photo_ref::NPIX, t.job[q].start_px, o.align, o.levels, recs);
        r[q] = recs[0];
    }
    if (edge_recs) memcpy(edge_recs, r.get(), sizeof(hnet_robust::Record) * ka::MAX_PAIRS);
    keyframe_adjust_ref_adjust_with(entries, m, r.get(), opts, record);
}

// the state's h_origin_key after an applied adjustment
void keyframe_adjust_ref_apply_state(const void* record, const void* opts, const void* map_state, int m, void* state) {
    ka::apply_state(*static_cast<const ka::Record*>(record), *static_cast<const ka::Opts*>(opts), *static_cast<const km::MapState*>(map_state), m,
                    *static_cast<kf::State*>(state));
}

void keyframe_adjust_ref_default_opts(void* opts) { ka::default_opts(*static_cast<ka::Opts*>(opts)); }
int keyframe_adjust_ref_opts_valid(const void* opts) { return ka::opts_valid(*static_cast<const ka::Opts*>(opts)) ? 1 : 0; }

}  // extern "C"

#ifdef KEYFRAME_ADJUST_REF_MAIN
// The header once over hostile inputs: entries and offsets that are NaN, infinite, huge, singular or invalid, rows that point outside the table, weights
// that are zero, NaN or negative, every capacity and every row count.  Checks what must hold whatever comes in: no written matrix is non-finite, and
// an untouched entry keeps its bytes.  Exit status 0, or 1 with a line per violation.
#include <cstdio>
#include <limits>

namespace {

uint64_t lcg(uint64_t& s) { return s = s * 6364136223846793005ull + 1442695040888963407ull; }
double unit(uint64_t& s) { return (double)(lcg(s) >> 11) / 9007199254740992.0; }

double hostile(uint64_t& s, double scale) {
    const int k = (int)(lcg(s) >> 60);
    if (k == 0) return std::numeric_limits<double>::quiet_NaN();
    if (k == 1) return std::numeric_limits<double>::infinity();
    if (k == 2) return -std::numeric_limits<double>::infinity();
    if (k == 3) return 1e300;
    if (k == 4) return 0.0;
    return (unit(s) - 0.5) * scale;
}

}  // namespace

int main() {
    uint64_t s = 12345;
    int bad = 0;
    std::unique_ptr<ka::Problem> P(new ka::Problem);
    for (int round = 0; round < 400; round++) {
        const int m = 1 + (int)(lcg(s) >> 61);                         // 1 .. 8
        km::Entry e[ka::MAX_ENTRIES], before[ka::MAX_ENTRIES];
        ka::Edge edges[ka::MAX_PAIRS];
        double infos[ka::MAX_PAIRS * 64];
        const bool wild = round % 3 == 0;
        for (int k = 0; k < m; k++) {
            e[k].valid = (lcg(s) >> 62) != 0;
            e[k].links = (int)(lcg(s) >> 60);
            e[k].serial = k + 1;
            e[k].pad = 0;
            for (int c = 0; c < 9; c++) {
                const double id = (c & 3) == 0 ? 1.0 : 0.0, sc = (c == 2 || c == 5) ? 60.0 : (c == 6 || c == 7) ? 1e-5 : 0.05;
                e[k].h_origin_key[c] = id + ((wild && (lcg(s) >> 61) == 0) ? hostile(s, 1e3) : (unit(s) - 0.5) * sc);
            }
            if (!wild) e[k].h_origin_key[8] = 1.0;
            before[k] = e[k];
        }
        const int n_edges = (int)(lcg(s) % (ka::MAX_PAIRS + 1));
        for (int q = 0; q < n_edges; q++) {
            ka::edge_zero(edges[q]);
            int i, j;
            if (!ka::pair_slots((int)(lcg(s) % ka::MAX_PAIRS), m, i, j) || (wild && (lcg(s) >> 61) == 0)) { i = (int)(lcg(s) >> 59) - 8; j = (int)(lcg(s) >> 59) - 8; }
            edges[q].i = i; edges[q].j = j;
            edges[q].flags = (lcg(s) >> 62) == 0 ? ka::EDGE_LOW_OVERLAP : ka::EDGE_ACCEPTED;
            edges[q].mse = wild ? hostile(s, 50.0) : unit(s) * 20.0;
            for (int k = 0; k < 8; k++) edges[q].offsets_px[k] = (float)((wild && (lcg(s) >> 61) == 0) ? hostile(s, 1e4) : (unit(s) - 0.5) * 80.0);
            for (int k = 0; k < 64; k++) {
                const double id = (k % 9) == 0 ? 1e4 * unit(s) : 0.0;
                infos[q * 64 + k] = (wild && (lcg(s) >> 60) == 0) ? hostile(s, 1e5) : id;
            }
        }
        ka::Opts o;
        ka::default_opts(o);
        o.weighting = (int)(lcg(s) >> 63);
        o.apply = (int)(lcg(s) >> 63);
        o.max_trials = 1 + (int)(lcg(s) % 12);
        o.max_shift_px = (lcg(s) >> 63) ? 5.0 : 0.0;
        ka::Record rec;
        memset(&rec, 0xA5, sizeof rec);
        seed(rec, n_edges, edges);
        ka::adjust_host(e, m, (lcg(s) >> 62) == 0 ? nullptr : infos, o, rec, *P);
        const bool adjusted = (rec.flags & ka::ADJ_ADJUSTED) != 0;
        for (int k = 0; k < m; k++) {
            const bool moved = adjusted && o.apply && ((rec.adjusted_mask >> k) & 1) && k != rec.anchor;
            if (!moved && memcmp(&e[k], &before[k], sizeof e[k]) != 0) { printf("round %d: entry %d changed without being adjusted\n", round, k); bad++; }
            if (e[k].valid != before[k].valid || e[k].links != before[k].links || e[k].serial != before[k].serial) { printf("round %d: bookkeeping of entry %d changed\n", round, k); bad++; }
            for (int c = 0; c < 9; c++) {
                if (moved && !std::isfinite(e[k].h_origin_key[c])) { printf("round %d: entry %d received a non-finite matrix\n", round, k); bad++; }
                if (adjusted && ((rec.adjusted_mask >> k) & 1) && !std::isfinite(rec.h_origin_key[k][c])) { printf("round %d: record matrix %d is not finite\n", round, k); bad++; }
                if (!(adjusted && ((rec.adjusted_mask >> k) & 1)) && memcmp(&rec.h_origin_key[k][c], &before[k].h_origin_key[c], sizeof(double)) != 0) {
                    printf("round %d: record matrix %d differs from an untouched entry\n", round, k);
                    bad++;
                }
            }
        }
        kf::State st;
        km::MapState ms;
        memset(&st, 0, sizeof st);
        ms.cur_slot = (int)(lcg(s) >> 59) - 12; ms.cur_links = 0; ms.cursor = 0; ms.serial = 0;
        ka::apply_state(rec, o, ms, m, st);
        for (int c = 0; c < 9; c++)
            if (!std::isfinite(st.h_origin_key[c])) { printf("round %d: the state received a non-finite matrix\n", round); bad++; }
        ka::JobTable t;
        ka::pairs(before, m, 1 + (int)(lcg(s) % 64), t);
        if (t.count < 0 || t.count > t.n_pairs || t.n_pairs > ka::MAX_PAIRS) { printf("round %d: job counts %d of %d\n", round, t.count, t.n_pairs); bad++; }
    }
    printf("keyframe_adjust_ref: %d violations\n", bad);
    return bad ? 1 : 0;
}
#endif
