/* hnet_keyframe_adjust.h — the JOINT ADJUSTMENT of a session's keyframe map (include/hnet.h hnet_op_keyframe_adjust_solve, hnet_op_keyframe_adjust,
 * hnet_sessions_keyframe_adjust): every overlapping pair of stored keyframes is re-measured by the robust alignment and all their places are
 * solved for at once, a small pose-graph adjustment over homographies (at most 8 nodes, 28 edges, 56 unknowns).  What the device
 * (csrc/kernels_keyframe_adjust.hip) and the host reference (tests/cpp/keyframe_adjust_ref.cpp) both compile, on top of include/hnet_keyframe_map.h
 * (Entry, relative, grid_count, inverse, corners) and include/hnet_keyframe.h (chain, mul3); the conventions are those headers': X_k = h_origin_key of
 * entry k maps origin -> keyframe k, H(x) maps a template pixel to the other image.
 *
 * PAIRS.  The slots i < j < m in lexicographic order, pair p of m (m - 1) / 2 (pair_slots).  Both entries must be USABLE: valid and with an inverse
 * (km::inverse).  relative(X_j, entry_i, G, start_px): G = X_j . inverse(X_i) maps a pixel of i into j.  A pair is a JOB when relative succeeds and
 * grid_count(G) >= min_grid; the template is image i, the other image j, the start start_px.  pairs() lists the jobs in pair order (JobTable).
 * EDGES.  judge_edge: a job's level-0 alignment record becomes a row of the edge table with ONE flag, tested in decide_revisit's order: EDGE_STOPPED (the
 * record stopped SINGULAR, DEGENERATE or FEW_PIXELS), EDGE_MSE_ABOVE_MAX (max_mse > 0 and not mse <= max_mse), EDGE_NON_FINITE (an offset of the record),
 * EDGE_LOW_OVERLAP (n_valid / 71 680 < min_overlap), EDGE_CLOSURE_ABOVE_MAX (max_closure_px > 0 and the worst |offset - start| exceeds it), else
 * EDGE_ACCEPTED.  Only accepted edges enter the solve.
 * BUILD.  build() turns entries [m] and an edge table into a Problem.  A row that says EDGE_ACCEPTED but cannot be one - i, j not i < j < m, an endpoint
 * that is not usable, a failed relative, an offset that is not finite - becomes EDGE_NO_RELATIVE (this can only happen to a caller-supplied table).  The
 * ANCHOR is the usable entry with the fewest links, then the lowest slot; it does not move.  The SET is the entries connected to the anchor through
 * accepted edges (the anchor included, adjusted_mask); usable entries outside it go into unconnected_mask and keep their bytes.  The solve's edges are the
 * accepted rows inside the set, in table order; the others are constants of the cost and are left out of it (their r0_px and r_px stay 0).
 * UNKNOWNS AND COST.  Every entry k of the set but the anchor has delta_k, 8 doubles: four-corner offsets in keyframe k's own pixels; its new matrix is
 * X_k' = chain(H(delta_k), X_k), H in double from double offsets (homography_d).  For edge (i, j): P = H(delta_j) . G . inverse(H(delta_i)),
 * r = (double) offsets_px - (corners(P) - p4), 8 numbers in pixels (edge_residual).  cost = sum over the solve's edges, in order, of r^T W r
 * (edge_cost: sum_a r[a] (sum_b W[a][b] r[b])).  W = I (WEIGHT_UNIT) or info / max(mse, mse_floor) (WEIGHT_INFO; info = I when the caller of the
 * solve-only form passes none).  An edge whose P has no corners has NaN residuals: the cost is not finite and the trial is refused.
 * JACOBIAN.  Analytic, one column per (edge, endpoint, component): jacobian_col, through hnet_align::dlt_jacobian_col (the derivative of dlt_solve);
 * central differences at 1e-4 px reach the same solutions.  The anchor's columns are zero and belong to no unknown.
 * SOLVE.  solve(): Levenberg-Marquardt like the alignment's.  A = sum_e J_e^T (W_e J_e), g = sum_e J_e^T (W_e r_e); every entry is summed by ONE task over
 * the edges in order (normal_entry, gradient_entry; the lower triangle is formed and mirrored).  A + lambda diag(A) is factorised column by column with
 * hnet_align::cholesky's sums and pivot test (a pivot <= 1e-12 max diag(A), or not finite: ADJ_SINGULAR, judged on the undamped matrix first, as
 * solve_damped does).  A trial is accepted when its cost is finite and <= the current cost: lambda / 10, else lambda x 10; every trial counts towards
 * max_trials.  ADJ_CONVERGED when the step proposed from the current point (reached by accepted steps) moves no component by eps_px or more: that step
 * is NOT tried.  Trying it would be a coin flip: one step after a step of 1e-4 px the proposal is about 1e-9 px, the cost changes in its last bits, and
 * whether the trial is accepted or refused - and so `trials`, `accepted` and `lambda` - would depend on the last bits of the alignments.
 * After a run of refusals the damping alone makes a step small: read cost against cost0 and lambda before taking CONVERGED for "adjusted".
 * The work is written against an executor `Par` with for_each(n, f) and single(f): the host's Serial runs the tasks one after the other, the device's
 * spreads them over the 256 lanes of a workgroup between barriers.  Every task's sums have one written order, so both give the same bits.
 * VERDICT, all or nothing per session (finish), tested in this order: ADJ_FEW_ENTRIES (fewer than two usable entries), ADJ_NO_EDGES (no accepted edge
 * reaches the anchor), ADJ_SINGULAR, ADJ_NO_GAIN (not cost < cost0), ADJ_SHIFT_ABOVE_MAX (max_shift_px > 0 and the worst |delta| exceeds it: the guard
 * against a false match, as max_closure_px is for a revisit), ADJ_CHAIN (a chain(H(delta_k), X_k) fails), else ADJ_ADJUSTED.  ADJ_CONVERGED rides along
 * with any of the last four.  The new matrices are written to the record only with ADJ_ADJUSTED (else the old ones); delta_px holds what the solve
 * reached whenever it ran.  With apply they are also written into the entries, and apply_state moves the state's h_origin_key with entry cur_slot's, so
 * that state.h_origin_key == entries[cur_slot].h_origin_key keeps holding.  valid, links, serial, the map state and the images are never touched.
 * Every body is non-contracting, everything is in double, nothing depends on the batch or the slot.
 */
#ifndef HNET_KEYFRAME_ADJUST_H
#define HNET_KEYFRAME_ADJUST_H

#include "hnet_keyframe_map.h"

namespace hnet_adjust {

namespace kf = hnet_keyframe;
namespace km = hnet_keyframe_map;
namespace pa = hnet_align;
namespace pr = hnet_robust;

constexpr int MAX_ENTRIES = km::MAX_CAPACITY, MAX_PAIRS = 28, NC = 8, JCOLS = 16, MAX_UNKNOWNS = NC * (MAX_ENTRIES - 1), MAX_TRIALS = 64;
constexpr double PIVOT_TINY = 1e-12, MAX_LAMBDA0 = 1e100;
static_assert(MAX_PAIRS == MAX_ENTRIES * (MAX_ENTRIES - 1) / 2, "every pair of slots");

/* the flags of an adjust record (= HNET_ADJ_*): one verdict, and CONVERGED beside it */
enum { ADJ_FEW_ENTRIES = 1, ADJ_NO_EDGES = 2, ADJ_SINGULAR = 4, ADJ_NO_GAIN = 8, ADJ_SHIFT_ABOVE_MAX = 16, ADJ_CHAIN = 32, ADJ_ADJUSTED = 64, ADJ_CONVERGED = 128 };
/* the flag of an edge (= HNET_ADJ_EDGE_*); 0: an unused row */
enum { EDGE_ACCEPTED = 1, EDGE_STOPPED = 2, EDGE_MSE_ABOVE_MAX = 4, EDGE_NON_FINITE = 8, EDGE_LOW_OVERLAP = 16, EDGE_CLOSURE_ABOVE_MAX = 32, EDGE_NO_RELATIVE = 64 };
enum { WEIGHT_UNIT = 0, WEIGHT_INFO = 1 };

/* = hnet_keyframe_adjust_opts */
struct Opts {
    pr::Opts align;
    int32_t levels, min_grid;
    double min_overlap, max_mse, max_closure_px;
    int32_t weighting, max_trials;
    double mse_floor, lambda0, eps_px, max_shift_px;
    int32_t apply, pad;
};
inline void default_opts(Opts& o) {
    pr::default_opts(o.align);
    o.levels = 3; o.min_grid = 32; o.min_overlap = 0.5; o.max_mse = 0.0; o.max_closure_px = 0.0;
    o.weighting = WEIGHT_INFO; o.max_trials = 24; o.mse_floor = 1.0; o.lambda0 = 1e-3; o.eps_px = 1e-6; o.max_shift_px = 0.0;
    o.apply = 0; o.pad = 0;
}
inline bool opts_valid(const Opts& o) {
    return pr::opts_valid(o.align) && o.levels >= 1 && o.levels <= pa::MAX_LEVELS && o.min_grid >= 1 && o.min_grid <= km::GRID_POINTS && o.min_overlap >= 0.0 &&
           o.min_overlap <= 1.0 && o.max_mse >= 0.0 && std::isfinite(o.max_mse) && o.max_closure_px >= 0.0 && std::isfinite(o.max_closure_px) &&
           (o.weighting == WEIGHT_UNIT || o.weighting == WEIGHT_INFO) && o.max_trials >= 1 && o.max_trials <= MAX_TRIALS && o.mse_floor > 0.0 &&
           std::isfinite(o.mse_floor) && o.lambda0 > 0.0 && o.lambda0 <= MAX_LAMBDA0 && o.eps_px >= 0.0 && std::isfinite(o.eps_px) && o.max_shift_px >= 0.0 &&
           std::isfinite(o.max_shift_px) && (o.apply == 0 || o.apply == 1);
}

/* one job: the pair, its grid count and the start of its alignment */
struct Job { int32_t i, j, grid, pad; float start_px[NC]; };
/* a session's jobs in pair order; unused rows are zero */
struct JobTable { int32_t count, n_pairs; Job job[MAX_PAIRS]; };
/* = hnet_keyframe_adjust_edge */
struct Edge { int32_t i, j, grid, flags; float start_px[NC], offsets_px[NC]; double mse, overlap, r0_px, r_px; };
/* = hnet_keyframe_adjust; every byte written, pad = 0 */
struct Record {
    int32_t flags, anchor, n_pairs, n_jobs, n_edges, adjusted_mask, unconnected_mask, trials, accepted, pad;
    double cost0, cost, lambda;
    double delta_px[MAX_ENTRIES][NC];
    double h_origin_key[MAX_ENTRIES][9];
    Edge edge[MAX_PAIRS];
};

/* pair p of m slots -> (i, j), i < j < m, in lexicographic order; false: there is no such pair */
inline bool pair_slots(int p, int m, int& i, int& j) {
    int k = p;
    for (i = 0; i + 1 < m; i++) {
        const int row = m - 1 - i;
        if (k < row) { j = i + 1 + k; return k >= 0; }
        k -= row;
    }
    i = j = 0;
    return false;
}

inline bool usable(const km::Entry& e) {
    double inv[9];
    return e.valid != 0 && km::inverse(e.h_origin_key, inv);
}

/* pair p of the entries [m]: 0 - no such pair or an endpoint is not usable; 1 - a pair, but no job; 2 - a job, written in full */
inline int pair_job(const km::Entry* e, int m, int p, int min_grid, Job& job) {
    HNET_ALIGN_NO_CONTRACT
    int i, j;
    if (!pair_slots(p, m, i, j) || !usable(e[i]) || !usable(e[j])) return 0;
    double G[9];
    float start[NC];
    if (!km::relative(e[j].h_origin_key, e[i], G, start)) return 1;
    const int grid = km::grid_count(G);
    if (grid < min_grid) return 1;
    job.i = i; job.j = j; job.grid = grid; job.pad = 0;
    for (int k = 0; k < NC; k++) job.start_px[k] = start[k];
    return 2;
}

inline void job_zero(Job& j) {
    j.i = j.j = j.grid = j.pad = 0;
    for (int k = 0; k < NC; k++) j.start_px[k] = 0.0f;
}

/* the job table of the entries [m], every byte written */
inline void pairs(const km::Entry* e, int m, int min_grid, JobTable& t) {
    t.count = t.n_pairs = 0;
    for (int p = 0; p < MAX_PAIRS; p++) job_zero(t.job[p]);
    for (int p = 0; p < MAX_PAIRS; p++) {
        Job jb;
        const int k = pair_job(e, m, p, min_grid, jb);
        if (k >= 1) t.n_pairs++;
        if (k == 2) t.job[t.count++] = jb;
    }
}

inline void edge_zero(Edge& e) {
    e.i = e.j = e.grid = e.flags = 0;
    for (int k = 0; k < NC; k++) e.start_px[k] = e.offsets_px[k] = 0.0f;
    e.mse = e.overlap = e.r0_px = e.r_px = 0.0;
}

/* a job's level-0 record -> its row of the edge table, every byte written */
inline void judge_edge(const Job& job, const pr::Record& rec, const Opts& o, Edge& e) {
    HNET_ALIGN_NO_CONTRACT
    const double overlap = (double)rec.px.n_valid / kf::FRAME_PIXELS;
    bool rec_finite = true;
    double worst = 0.0;
    for (int k = 0; k < NC; k++) {
        rec_finite = rec_finite && std::isfinite(rec.px.offsets_px[k]);
        const double d = std::fabs((double)rec.px.offsets_px[k] - (double)job.start_px[k]);
        worst = d > worst ? d : worst;
    }
    int flags;
    if (rec.px.flags & (pa::SINGULAR | pa::DEGENERATE | pa::FEW_PIXELS)) flags = EDGE_STOPPED;
    else if (o.max_mse > 0.0 && !(rec.px.mse <= o.max_mse)) flags = EDGE_MSE_ABOVE_MAX;
    else if (!rec_finite) flags = EDGE_NON_FINITE;
    else if (overlap < o.min_overlap) flags = EDGE_LOW_OVERLAP;
    else if (o.max_closure_px > 0.0 && !(worst <= o.max_closure_px)) flags = EDGE_CLOSURE_ABOVE_MAX;
    else flags = EDGE_ACCEPTED;
    e.i = job.i; e.j = job.j; e.grid = job.grid; e.flags = flags;
    for (int k = 0; k < NC; k++) { e.start_px[k] = job.start_px[k]; e.offsets_px[k] = rec.px.offsets_px[k]; }
    e.mse = rec.px.mse; e.overlap = overlap; e.r0_px = 0.0; e.r_px = 0.0;
}

/* H(d) in double from double offsets; false when an offset or an entry of H is not finite */
inline bool homography_d(const double* d, double h[9]) {
    HNET_ALIGN_NO_CONTRACT
    double dst[8];
    bool ok = true;
    for (int k = 0; k < 8; k++) {
        dst[k] = hnet::p4(k) + d[k];
        ok = ok && std::isfinite(dst[k]);
    }
    hnet::dlt_solve(dst, h);
    for (int k = 0; k < 9; k++) ok = ok && std::isfinite(h[k]);
    return ok;
}

/* r = z - (corners(H(dj) . G . inverse(H(di))) - p4); false, and r = NaN, when P has no corners */
inline bool edge_residual(const double G[9], const double* di, const double* dj, const double* z, double r[NC]) {
    HNET_ALIGN_NO_CONTRACT
    double hi[9], hj[9], inv[9], t[9], P[9], c[8];
    bool ok = homography_d(di, hi) && homography_d(dj, hj) && km::inverse(hi, inv);
    if (ok) {
        kf::mul3(G, inv, t);
        kf::mul3(hj, t, P);
        ok = km::corners(P, c);
    }
    for (int k = 0; k < NC; k++) {
        r[k] = ok ? z[k] - c[k] : (double)kf::quiet_nan();
        ok = ok && std::isfinite(r[k]);
    }
    if (!ok)
        for (int k = 0; k < NC; k++) r[k] = (double)kf::quiet_nan();
    return ok;
}

/* wr = W r and r^T wr */
inline double edge_cost(const double* W, const double* r, double wr[NC]) {
    HNET_ALIGN_NO_CONTRACT
    double c = 0.0;
    for (int a = 0; a < NC; a++) {
        double s = 0.0;
        for (int b = 0; b < NC; b++) s += W[a * NC + b] * r[b];
        wr[a] = s;
    }
    for (int a = 0; a < NC; a++) c += r[a] * wr[a];
    return c;
}

/* column comp of d r / d delta of endpoint `which` (0: i, 1: j), analytic: with D = d H(delta) / d delta[comp] (hnet_align::dlt_jacobian_col, the
 * derivative of dlt_solve in double), dP = D . G . inverse(H_i) for endpoint j and dP = -P . D . inverse(H_i) for endpoint i, and a corner
 * (X / Z, Y / Z) of P moves by ((dX - x dZ) / Z, (dY - y dZ) / Z); r = z - corner, so the column is minus that.  NaN when P has no corners. */
inline void jacobian_col(const double G[9], const double* di, const double* dj, int which, int comp, double col[NC]) {
    HNET_ALIGN_NO_CONTRACT
    double hi[9], hj[9], inv[9], t[9], P[9], c[8], dst[8], D[9], dP[9], u9[9];
    bool ok = homography_d(di, hi) && homography_d(dj, hj) && km::inverse(hi, inv);
    if (ok) {
        kf::mul3(G, inv, t);
        kf::mul3(hj, t, P);
        ok = km::corners(P, c);
    }
    if (!ok) {
        for (int k = 0; k < NC; k++) col[k] = (double)kf::quiet_nan();
        return;
    }
    const double* d = which ? dj : di;
    for (int k = 0; k < 8; k++) dst[k] = hnet::p4(k) + d[k];
    pa::dlt_jacobian_col(dst, comp, D);
    if (which) {
        kf::mul3(D, t, dP);
    } else {
        kf::mul3(D, inv, u9);
        kf::mul3(P, u9, dP);
        for (int k = 0; k < 9; k++) dP[k] = -dP[k];
    }
    for (int q = 0; q < 4; q++) {
        const double u = hnet::p4(2 * q), v = hnet::p4(2 * q + 1);
        const double Z = (P[6] * u + P[7] * v) + P[8];
        const double dX = (dP[0] * u + dP[1] * v) + dP[2], dY = (dP[3] * u + dP[4] * v) + dP[5], dZ = (dP[6] * u + dP[7] * v) + dP[8];
        const double x = c[2 * q] + u, y = c[2 * q + 1] + v;
        col[2 * q] = -((dX - x * dZ) / Z);
        col[2 * q + 1] = -((dY - y * dZ) / Z);
    }
}

/* One session's adjustment.  On the device it lives in the workgroup's LDS. */
struct Problem {
    int32_t m, n_solve, n_unknown, anchor, usable_mask, set_mask, flags, trials, accepted, stop, fail, need_lin, n_edges, pad;
    int32_t unknown_of[MAX_ENTRIES];       /* node -> its block of 8 unknowns, or -1 (the anchor, or outside the set) */
    int32_t node_of[MAX_ENTRIES];          /* block -> node */
    int32_t ei[MAX_PAIRS], ej[MAX_PAIRS], row[MAX_PAIRS];      /* the solve's edges: endpoints and row of the edge table */
    double cost0, cost, cost_t, lambda, top, step_top;
    double G[MAX_PAIRS][9], z[MAX_PAIRS][NC], W[MAX_PAIRS][NC * NC];
    double delta[MAX_ENTRIES][NC], trial[MAX_ENTRIES][NC];
    double r[MAX_PAIRS][NC], rt[MAX_PAIRS][NC], wr[MAX_PAIRS][NC], r0_top[MAX_PAIRS], ce[MAX_PAIRS];
    double J[MAX_PAIRS][NC][JCOLS], WJ[MAX_PAIRS][NC][JCOLS];
    double A[MAX_UNKNOWNS * MAX_UNKNOWNS], L[MAX_UNKNOWNS * MAX_UNKNOWNS], g[MAX_UNKNOWNS], dx[MAX_UNKNOWNS];
};

/* entries [m], the edge table of rec (rec.n_jobs rows) and, for WEIGHT_INFO, infos [rows][64] (null: identity) -> the Problem and the record's anchor,
 * masks, n_pairs and n_edges.  P.flags: ADJ_FEW_ENTRIES, ADJ_NO_EDGES or 0 (the solve has something to do).  One task. */
inline void build(const km::Entry* e, int m, const double* infos, const Opts& o, Record& rec, Problem& P) {
    HNET_ALIGN_NO_CONTRACT
    P.m = m; P.n_solve = 0; P.n_unknown = 0; P.anchor = -1; P.usable_mask = 0; P.set_mask = 0; P.flags = 0; P.trials = 0; P.accepted = 0; P.stop = 0;
    P.fail = 0; P.need_lin = 1; P.n_edges = 0; P.pad = 0;
    P.cost0 = P.cost = P.cost_t = 0.0; P.lambda = o.lambda0; P.top = 0.0; P.step_top = 0.0;
    int n_usable = 0;
    for (int k = 0; k < MAX_ENTRIES; k++) {
        P.unknown_of[k] = -1;
        P.node_of[k] = 0;
        for (int c = 0; c < NC; c++) P.delta[k][c] = P.trial[k][c] = 0.0;
        if (k < m && usable(e[k])) {
            P.usable_mask |= 1 << k;
            n_usable++;
            if (P.anchor < 0 || e[k].links < e[P.anchor].links) P.anchor = k;
        }
    }
    int rows = rec.n_jobs;
    rows = rows < 0 ? 0 : rows > MAX_PAIRS ? MAX_PAIRS : rows;
    rec.n_jobs = rows;
    rec.n_pairs = n_usable * (n_usable - 1) / 2;
    rec.anchor = P.anchor;
    /* the rows that can be edges */
    for (int q = 0; q < rows; q++) {
        Edge& ed = rec.edge[q];
        ed.r0_px = ed.r_px = 0.0;
        if (ed.flags != EDGE_ACCEPTED) continue;
        bool ok = ed.i >= 0 && ed.i < ed.j && ed.j < m && ((P.usable_mask >> ed.i) & 1) && ((P.usable_mask >> ed.j) & 1);
        for (int k = 0; k < NC; k++) ok = ok && std::isfinite(ed.offsets_px[k]);
        if (ok) P.n_edges++;
        else ed.flags = EDGE_NO_RELATIVE;
    }
    /* G of every accepted row, into the slot the row would take as a solve edge: filled below once the set is known; first the rows' relatives */
    int n_rel = 0;
    for (int q = 0; q < rows; q++) {
        Edge& ed = rec.edge[q];
        if (ed.flags != EDGE_ACCEPTED) continue;
        float start[NC];
        if (!km::relative(e[ed.j].h_origin_key, e[ed.i], P.G[n_rel], start)) {
            ed.flags = EDGE_NO_RELATIVE;
            P.n_edges--;
            continue;
        }
        P.row[n_rel++] = q;
    }
    rec.n_edges = P.n_edges;
    if (n_usable < 2) {
        P.flags = ADJ_FEW_ENTRIES;
        rec.adjusted_mask = 0;
        rec.unconnected_mask = 0;
        return;
    }
    /* the set: what accepted edges connect to the anchor */
    P.set_mask = 1 << P.anchor;
    for (int pass = 0; pass < MAX_ENTRIES; pass++)
        for (int a = 0; a < n_rel; a++) {
            const Edge& ed = rec.edge[P.row[a]];
            const int bi = (P.set_mask >> ed.i) & 1, bj = (P.set_mask >> ed.j) & 1;
            if (bi != bj) P.set_mask |= (1 << ed.i) | (1 << ed.j);
        }
    rec.adjusted_mask = P.set_mask;
    rec.unconnected_mask = P.usable_mask & ~P.set_mask;
    for (int k = 0; k < m; k++)
        if (((P.set_mask >> k) & 1) && k != P.anchor) {
            P.unknown_of[k] = P.n_unknown;
            P.node_of[P.n_unknown++] = k;
        }
    /* the solve's edges, compacted in table order (G moves down with them) */
    for (int a = 0; a < n_rel; a++) {
        const int q = P.row[a];
        const Edge& ed = rec.edge[q];
        if (!((P.set_mask >> ed.i) & 1)) continue;
        const int s = P.n_solve++;
        for (int k = 0; k < 9; k++) P.G[s][k] = P.G[a][k];
        P.row[s] = q; P.ei[s] = ed.i; P.ej[s] = ed.j;
        for (int k = 0; k < NC; k++) P.z[s][k] = (double)ed.offsets_px[k];
        const double den = ed.mse > o.mse_floor ? ed.mse : o.mse_floor;
        for (int k = 0; k < NC * NC; k++) {
            const double id = (k % (NC + 1)) == 0 ? 1.0 : 0.0;
            P.W[s][k] = o.weighting == WEIGHT_UNIT ? id : (infos ? infos[(size_t)q * NC * NC + k] : id) / den;
        }
    }
    if (P.n_solve == 0) P.flags = ADJ_NO_EDGES;
}

/* entry (p, q), q <= p, of A: one task, the edges in order */
inline double normal_entry(const Problem& P, int p, int q) {
    HNET_ALIGN_NO_CONTRACT
    const int na = P.node_of[p >> 3], nb = P.node_of[q >> 3], ca = p & 7, cb = q & 7;
    double s = 0.0;
    for (int e = 0; e < P.n_solve; e++) {
        const int i = P.ei[e], j = P.ej[e];
        if ((na != i && na != j) || (nb != i && nb != j)) continue;
        const int cola = (na == i ? 0 : NC) + ca, colb = (nb == i ? 0 : NC) + cb;
        double t = 0.0;
        for (int k = 0; k < NC; k++) t += P.J[e][k][cola] * P.WJ[e][k][colb];
        s += t;
    }
    return s;
}
inline double gradient_entry(const Problem& P, int p) {
    HNET_ALIGN_NO_CONTRACT
    const int na = P.node_of[p >> 3], ca = p & 7;
    double s = 0.0;
    for (int e = 0; e < P.n_solve; e++) {
        const int i = P.ei[e], j = P.ej[e];
        if (na != i && na != j) continue;
        const int cola = (na == i ? 0 : NC) + ca;
        double t = 0.0;
        for (int k = 0; k < NC; k++) t += P.J[e][k][cola] * P.wr[e][k];
        s += t;
    }
    return s;
}

/* the host's executor: the tasks one after the other */
struct Serial {
    template <class F> void for_each(int n, F f) { for (int t = 0; t < n; t++) f(t); }
    template <class F> void single(F f) { f(); }
};

/* Cholesky of A + lambda diag(A) over N unknowns, column by column, into P.L; P.fail = 1 at a pivot <= tiny or not finite.  Task t of column j forms the
 * pivot d in hnet_align::cholesky's order (every task the same bits) and element j + t of the column. */
template <class Par>
inline void cholesky(Problem& P, int N, double lambda, double tiny, Par& par) {
    constexpr int S = MAX_UNKNOWNS;
    par.single([&] { P.fail = 0; });
    for (int j = 0; j < N; j++) {
        par.for_each(N - j, [&](int t) {
            HNET_ALIGN_NO_CONTRACT
            double d = P.A[j * S + j] + lambda * P.A[j * S + j];
            for (int k = 0; k < j; k++) d -= P.L[j * S + k] * P.L[j * S + k];
            const bool bad = !(d > tiny) || !std::isfinite(d);
            const double ljj = std::sqrt(d);
            if (t == 0) {
                P.L[j * S + j] = ljj;
                if (bad) P.fail = 1;
                return;
            }
            const int i = j + t;
            double s = P.A[i * S + j];
            for (int k = 0; k < j; k++) s -= P.L[i * S + k] * P.L[j * S + k];
            P.L[i * S + j] = s / ljj;
        });
        if (P.fail) return;                /* (read after the executor's barrier: uniform) */
    }
}

/* residuals and cost at the deltas `d` ([MAX_ENTRIES][NC]) into r / ce, the sum into *cost */
template <class Par>
inline void evaluate(Problem& P, double (*d)[NC], double (*r)[NC], double* cost, Par& par) {
    par.for_each(P.n_solve, [&](int e) {
        double wr[NC];
        edge_residual(P.G[e], d[P.ei[e]], d[P.ej[e]], P.z[e], r[e]);
        P.ce[e] = edge_cost(P.W[e], r[e], wr);
    });
    par.single([&] {
        HNET_ALIGN_NO_CONTRACT
        double c = 0.0;
        for (int e = 0; e < P.n_solve; e++) c += P.ce[e];
        *cost = c;
    });
}

/* the Levenberg-Marquardt loop on a built Problem with P.flags == 0: P.delta, P.r, cost0, cost, lambda, trials, accepted, and ADJ_SINGULAR /
 * ADJ_CONVERGED into P.flags */
template <class Par>
inline void solve(Problem& P, const Opts& o, Par& par) {
    constexpr int S = MAX_UNKNOWNS;
    const int N = NC * P.n_unknown, E = P.n_solve;
    evaluate(P, P.delta, P.r, &P.cost, par);
    par.single([&] {
        HNET_ALIGN_NO_CONTRACT
        P.cost0 = P.cost;
        for (int e = 0; e < E; e++) {
            double top = 0.0;
            for (int k = 0; k < NC; k++) {
                const double a = std::fabs(P.r[e][k]);
                top = a > top ? a : top;
            }
            P.r0_top[e] = top;
        }
        if (!std::isfinite(P.cost0)) P.stop = 1;       /* nothing to descend from: the verdict is ADJ_NO_GAIN */
    });
    while (!P.stop) {
        if (P.need_lin) {
            par.for_each(E * JCOLS, [&](int t) {
                const int e = t / JCOLS, col = t % JCOLS, which = col / NC;
                double c[NC];
                if (P.unknown_of[which ? P.ej[e] : P.ei[e]] < 0) {
                    for (int k = 0; k < NC; k++) c[k] = 0.0;
                } else {
                    jacobian_col(P.G[e], P.delta[P.ei[e]], P.delta[P.ej[e]], which, col % NC, c);
                }
                for (int k = 0; k < NC; k++) P.J[e][k][col] = c[k];
            });
            par.for_each(E * JCOLS, [&](int t) {
                HNET_ALIGN_NO_CONTRACT
                const int e = t / JCOLS, col = t % JCOLS;
                for (int k = 0; k < NC; k++) {
                    double s = 0.0;
                    for (int l = 0; l < NC; l++) s += P.W[e][k * NC + l] * P.J[e][l][col];
                    P.WJ[e][k][col] = s;
                }
                if (col == 0) edge_cost(P.W[e], P.r[e], P.wr[e]);
            });
            par.for_each(N * (N + 1) / 2 + N, [&](int t) {
                const int tri = N * (N + 1) / 2;
                if (t >= tri) {
                    P.g[t - tri] = gradient_entry(P, t - tri);
                    return;
                }
                int p = 0, k = t;
                while (k > p) { k -= p + 1; p++; }      /* t -> (p, q), q <= p, by rows of the lower triangle */
                const double a = normal_entry(P, p, k);
                P.A[p * S + k] = a;
                P.A[k * S + p] = a;
            });
            par.single([&] {
                double top = 0.0;
                for (int i = 0; i < N; i++) top = P.A[i * S + i] > top ? P.A[i * S + i] : top;
                P.top = top;
            });
            const double tiny0 = PIVOT_TINY * P.top;
            if (!std::isfinite(tiny0)) {
                par.single([&] { P.fail = 1; });
            } else {
                cholesky(P, N, 0.0, tiny0, par);
            }
            if (P.fail) {
                par.single([&] { P.flags |= ADJ_SINGULAR; P.stop = 1; });
                break;
            }
        }
        cholesky(P, N, P.lambda, PIVOT_TINY * P.top, par);
        if (P.fail) {
            par.single([&] { P.flags |= ADJ_SINGULAR; P.stop = 1; });
            break;
        }
        par.single([&] {
            HNET_ALIGN_NO_CONTRACT
            for (int i = 0; i < N; i++) {                       /* L y = -g, y in dx */
                double s = -P.g[i];
                for (int k = 0; k < i; k++) s -= P.L[i * S + k] * P.dx[k];
                P.dx[i] = s / P.L[i * S + i];
            }
            for (int i = N - 1; i >= 0; i--) {                  /* L^T dx = y, in place */
                double s = P.dx[i];
                for (int k = i + 1; k < N; k++) s -= P.L[k * S + i] * P.dx[k];
                P.dx[i] = s / P.L[i * S + i];
            }
            bool ok = true;
            double top = 0.0;
            for (int i = 0; i < N; i++) {
                ok = ok && std::isfinite(P.dx[i]);
                const double a = std::fabs(P.dx[i]);
                top = a > top ? a : top;
                P.trial[P.node_of[i >> 3]][i & 7] = P.delta[P.node_of[i >> 3]][i & 7] + P.dx[i];
            }
            P.step_top = top;
            P.fail = ok ? 0 : 1;
            if (ok && top < o.eps_px) { P.flags |= ADJ_CONVERGED; P.stop = 1; }       /* a step this small is not tried */
        });
        if (P.fail) {
            par.single([&] { P.flags |= ADJ_SINGULAR; P.stop = 1; });
            break;
        }
        if (P.stop) break;
        evaluate(P, P.trial, P.rt, &P.cost_t, par);
        par.single([&] {
            HNET_ALIGN_NO_CONTRACT
            P.trials++;
            if (std::isfinite(P.cost_t) && P.cost_t <= P.cost) {
                P.accepted++;
                P.lambda = P.lambda / 10.0;
                P.cost = P.cost_t;
                for (int i = 0; i < N; i++) P.delta[P.node_of[i >> 3]][i & 7] = P.trial[P.node_of[i >> 3]][i & 7];
                for (int e = 0; e < E; e++)
                    for (int k = 0; k < NC; k++) P.r[e][k] = P.rt[e][k];
                P.need_lin = 1;
            } else {
                P.lambda = P.lambda * 10.0;
                P.need_lin = 0;
            }
            if (P.trials >= o.max_trials) P.stop = 1;
        });
    }
}

/* the verdict and the record's fields after build (and solve, when P.flags was 0): one task.  With o.apply and ADJ_ADJUSTED the new matrices are written
 * into e [m] too.  rec.edge, n_jobs, n_pairs, n_edges, anchor and the masks are build's. */
inline void finish(const Problem& P, const Opts& o, km::Entry* e, int m, Record& rec) {
    HNET_ALIGN_NO_CONTRACT
    int flags = P.flags & (ADJ_FEW_ENTRIES | ADJ_NO_EDGES);
    const bool ran = flags == 0;
    if (ran) {
        flags = P.flags & ADJ_CONVERGED;
        double worst = 0.0;
        bool chained = true;
        for (int u = 0; u < P.n_unknown; u++) {            /* every chain is formed twice, here for the verdict and below for the matrix: no table of them */
            const int k = P.node_of[u];
            double hd[9], hn[9];
            for (int c = 0; c < NC; c++) {
                const double a = std::fabs(P.delta[k][c]);
                worst = a > worst ? a : worst;
            }
            chained = chained && homography_d(P.delta[k], hd) && kf::chain(hd, e[k].h_origin_key, hn);
        }
        if (P.flags & ADJ_SINGULAR) flags = ADJ_SINGULAR | (flags & ADJ_CONVERGED);
        else if (!(P.cost < P.cost0)) flags |= ADJ_NO_GAIN;
        else if (o.max_shift_px > 0.0 && !(worst <= o.max_shift_px)) flags |= ADJ_SHIFT_ABOVE_MAX;
        else if (!chained) flags |= ADJ_CHAIN;
        else flags |= ADJ_ADJUSTED;
    }
    const bool adjusted = (flags & ADJ_ADJUSTED) != 0;
    rec.flags = flags;
    rec.trials = P.trials; rec.accepted = P.accepted; rec.pad = 0;
    rec.cost0 = ran ? P.cost0 : 0.0; rec.cost = ran ? P.cost : 0.0; rec.lambda = P.lambda;
    for (int k = 0; k < MAX_ENTRIES; k++) {
        for (int c = 0; c < NC; c++) rec.delta_px[k][c] = ran ? P.delta[k][c] : 0.0;
        for (int c = 0; c < 9; c++) rec.h_origin_key[k][c] = k < m ? e[k].h_origin_key[c] : 0.0;
    }
    if (ran)
        for (int s = 0; s < P.n_solve; s++) {
            double top = 0.0;
            for (int k = 0; k < NC; k++) {
                const double a = std::fabs(P.r[s][k]);
                top = a > top ? a : top;
            }
            rec.edge[P.row[s]].r0_px = P.r0_top[s];
            rec.edge[P.row[s]].r_px = top;
        }
    if (adjusted)
        for (int u = 0; u < P.n_unknown; u++) {
            const int k = P.node_of[u];
            double hd[9], hn[9];
            homography_d(P.delta[k], hd);
            kf::chain(hd, e[k].h_origin_key, hn);
            for (int c = 0; c < 9; c++) {
                rec.h_origin_key[k][c] = hn[c];
                if (o.apply) e[k].h_origin_key[c] = hn[c];
            }
        }
}

/* after finish with apply: the state's h_origin_key follows entry cur_slot's when that entry was moved */
inline void apply_state(const Record& rec, const Opts& o, const km::MapState& ms, int m, kf::State& s) {
    if (!o.apply || !(rec.flags & ADJ_ADJUSTED) || ms.cur_slot < 0 || ms.cur_slot >= m) return;
    if (!((rec.adjusted_mask >> ms.cur_slot) & 1) || ms.cur_slot == rec.anchor) return;
    for (int c = 0; c < 9; c++) s.h_origin_key[c] = rec.h_origin_key[ms.cur_slot][c];
}

/* every byte of a record that the edge table does not hold, zeroed (before the rows are written) */
inline void record_zero(Record& rec) {
    rec.flags = rec.anchor = rec.n_pairs = rec.n_jobs = rec.n_edges = rec.adjusted_mask = rec.unconnected_mask = rec.trials = rec.accepted = rec.pad = 0;
    rec.cost0 = rec.cost = rec.lambda = 0.0;
    for (int k = 0; k < MAX_ENTRIES; k++) {
        for (int c = 0; c < NC; c++) rec.delta_px[k][c] = 0.0;
        for (int c = 0; c < 9; c++) rec.h_origin_key[k][c] = 0.0;
    }
    for (int q = 0; q < MAX_PAIRS; q++) edge_zero(rec.edge[q]);
}

/* the whole solve of one session on the host: rec holds the edge table and n_jobs */
inline void adjust_host(km::Entry* e, int m, const double* infos, const Opts& o, Record& rec, Problem& P) {
    Serial par;
    build(e, m, infos, o, rec, P);
    if (P.flags == 0) solve(P, o, par);
    finish(P, o, e, m, rec);
}

}  /* namespace hnet_adjust */

#endif /* HNET_KEYFRAME_ADJUST_H */
