"""The cases that tests/test_keyframe_adjust_hostile_cpu.py and tests/test_gpu_keyframe_adjust_hostile.py share (include/hnet_keyframe_adjust.h; DESIGN
7ad): a float64 Gauss-Newton written from the statement of the problem (np_minimise: central differences, numpy lstsq - nothing of the header's), the
inconsistent-edge inputs, the asymmetric triangle, the input whose trials are refused, maps far from the origin, inputs for the singular exits, tables for
every shape of the index maps, the generator of the reference's stand-alone driver restated in Python, and the comparison of two records that lets two
NaNs be equal.  The gates are measured on the host reference (the CPU test file prints the figures; DESIGN 7ad holds them)."""
import functools

import numpy as np

import keyframe_adjust_util as A
import keyframe_render_util as R
import keyframe_util as K
from cuahn_vio_amd import _capi

UNIT, INFO = _capi.ADJ_WEIGHT_UNIT, _capi.ADJ_WEIGHT_INFO
ACCEPTED, LOW_OVERLAP = _capi.ADJ_EDGE_ACCEPTED, _capi.ADJ_EDGE_LOW_OVERLAP
ADJUSTED, CONVERGED, SINGULAR, NO_GAIN = _capi.ADJ_ADJUSTED, _capi.ADJ_CONVERGED, _capi.ADJ_SINGULAR, _capi.ADJ_NO_GAIN

# |delta_px - np_minimise| over the inconsistent cases and the triangle on the host reference: the worst is MINIMUM_WORST px (ring-8 seed 0, +-0.5 px, UNIT
# weights; DESIGN 7ad holds every case).  The floor is np_minimise's own: its finite-difference Jacobian moves its fixed point.  The gate is ten times the
# worst and far below 1e-4 px, 7q's host / device margin.
MINIMUM_WORST = 1.10e-7
MINIMUM_GATE = 10 * MINIMUM_WORST
COST_RTOL = 1e-9
# jacobian_col against central differences of edge_residual, relative to the column's largest entry: the worst over every column, point and G at the best
# step.  The gate is ten times it; a wrong sign or a swapped endpoint misses by order 1.
JACOBIAN_WORST = 3.54e-10
JACOBIAN_GATE = 10 * JACOBIAN_WORST
# far maps on the host reference: the worst |delta_px far - near| per shift over all-8 and ring-8, seeds 0 - 3; the gate is ten times it
FAR_SHIFTS = (1e5, 1e6)
FAR_DELTA_WORST = {1e5: 1.04e-10, 1e6: 9.13e-10}
FAR_GATE_FACTOR = 10


def infos_spd(n, seed):
    """symmetric positive definite 8 x 8 matrices of the size an alignment's information has (as tests/test_gpu_keyframe_adjust.py draws them)"""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, 8, 8))
    return (a @ a.transpose(0, 2, 1) + 8.0 * np.eye(8)) * 50.0


def weights(rows, weighting, infos, mse_floor=1.0):
    """W [n, 8, 8] as the statement of the cost has them: I, or info / max(mse, mse_floor) (info = I when there are no matrices)"""
    n = len(rows)
    if weighting == UNIT:
        return np.tile(np.eye(8), (n, 1, 1))
    inf = np.tile(np.eye(8), (n, 1, 1)) if infos is None else np.asarray(infos, np.float64).reshape(n, 8, 8)
    return inf / np.maximum(np.asarray(rows["mse"], np.float64), mse_floor)[:, None, None]


# ---- an independent minimiser

def _setup(ent, rows):
    e, ed = np.asarray(ent).reshape(-1), np.asarray(rows).reshape(-1)
    x = [np.asarray(k["h_origin_key"], np.float64) for k in e]
    prs = [(int(r["i"]), int(r["j"])) for r in ed]
    g = [x[j] @ np.linalg.inv(x[i]) for i, j in prs]
    z = [np.asarray(r["offsets_px"], np.float64) for r in ed]
    return len(e), prs, g, z


def np_residuals(ent, rows, d):
    """r_e = z_e - corners(H(d_j) . X_j X_i^-1 . H(d_i)^-1) of every row -> [n, 8] float64"""
    m, prs, g, z = _setup(ent, rows)
    hs = [K.homography(d[k]) for k in range(m)]
    return np.stack([z[q] - K.corners(hs[j] @ g[q] @ np.linalg.inv(hs[i])) for q, (i, j) in enumerate(prs)])


def np_cost(ent, rows, W, d):
    r = np_residuals(ent, rows, d)
    return float(sum(r[q] @ W[q] @ r[q] for q in range(len(r))))


def np_minimise(ent, rows, W, anchor, step=1e-4, tol=1e-12, max_iter=60):
    """the minimum of sum_e r_e^T W_e r_e over d_k (8 per entry, d_anchor = 0), every row an edge of the problem: a plain float64 Gauss-Newton on the
    residuals whitened by the Cholesky factors of W, the Jacobian by central differences (one entry's 8 unknowns at a time, only that entry's edges
    evaluated again), the step by numpy lstsq and halved while the cost would rise -> (d [m, 8], cost)"""
    m, prs, g, z = _setup(ent, rows)
    lt = [np.linalg.cholesky(np.asarray(W[q], np.float64)).T for q in range(len(prs))]                     # W = L L^T: |L^T r|^2 = r^T W r
    free = [k for k in range(m) if k != anchor]
    col = {k: 8 * n for n, k in enumerate(free)}
    touching = {k: [q for q, p in enumerate(prs) if k in p] for k in free}

    def one(q, hi_inv, hj):
        return lt[q] @ (z[q] - K.corners(hj @ g[q] @ hi_inv))

    def everything(d):
        hs = [K.homography(d[k]) for k in range(m)]
        his = [np.linalg.inv(h) for h in hs]
        return hs, his, np.concatenate([one(q, his[i], hs[j]) for q, (i, j) in enumerate(prs)])

    d = np.zeros((m, 8))
    hs, his, r = everything(d)
    for _ in range(max_iter):
        jac = np.zeros((8 * len(prs), 8 * len(free)))
        for k in free:
            for c in range(8):
                side = []
                for s in (step, -step):
                    v = d[k].copy()
                    v[c] += s
                    hk = K.homography(v)
                    hki = np.linalg.inv(hk)
                    side.append([one(q, hki if prs[q][0] == k else his[prs[q][0]], hk if prs[q][1] == k else hs[prs[q][1]]) for q in touching[k]])
                for n, q in enumerate(touching[k]):
                    jac[8 * q:8 * q + 8, col[k] + c] = (side[0][n] - side[1][n]) / (2.0 * step)
        dx = np.linalg.lstsq(jac, -r, rcond=None)[0].reshape(len(free), 8)
        scale = 1.0
        while True:
            t = d.copy()
            t[free] += scale * dx
            ths, this, tr = everything(t)
            if tr @ tr <= r @ r or scale < 1e-6:
                break
            scale *= 0.5
        moved = float(np.abs(scale * dx).max())
        if tr @ tr <= r @ r:
            d, hs, his, r = t, ths, this, tr
        if moved < tol:
            break
    return d, float(r @ r)


# ---- inconsistent edges

NOISES = (0.5, 5.0)
INCONSISTENT = tuple((name, seed, noise, w) for name in ("all-3", "all-8", "ring-8") for seed in (0, 1) for noise in NOISES for w in (UNIT, INFO))
TIGHT = dict(eps_px=1e-9, max_trials=64)                                     # so that the rule's own stopping distance is not what is measured


@functools.lru_cache(maxsize=None)
def inconsistent_case(name, seed, noise, weighting):
    """exact_case(name, seed) with its edge offsets perturbed by uniform +-noise px (fp32), mse in 0.2 .. 30 and, for INFO, matrices of an alignment's
    size -> (entries, rows, infos or None)"""
    truths, ent, ed = A.exact_case(name, seed)
    rows = np.array(ed)
    rows["offsets_px"] = (rows["offsets_px"] + np.random.default_rng(5).uniform(-noise, noise, rows["offsets_px"].shape)).astype(np.float32)
    rows["mse"] = np.random.default_rng(seed).uniform(0.2, 30.0, len(ed))
    rows.setflags(write=False)
    return ent, rows, infos_spd(len(ed), seed) if weighting == INFO else None


@functools.lru_cache(maxsize=None)
def triangle_case():
    """a triangle in which only edge (1, 2) contradicts the others, its W = diag(1, 2, 4 .. 128), the anchor slot 1: endpoint i of (0, 1) and endpoint j
    of (1, 2) are the free ones, and (0, 2) has both -> (entries, rows, infos)"""
    truths, ent, ed = A.exact_case("all-3", 1)
    e, rows = np.array(ent), np.array(ed)
    e["links"] = [1, 0, 2]
    rows["offsets_px"][2] += np.array([3.0, -2.0, 1.5, 2.5, -3.0, 1.0, -1.5, 2.0], np.float32)
    infos = np.tile(np.eye(8), (3, 1, 1))
    infos[2] = np.diag(2.0 ** np.arange(8))
    e.setflags(write=False)
    rows.setflags(write=False)
    return e, rows, infos


@functools.lru_cache(maxsize=None)
def minimum(key):
    """np_minimise of an inconsistent case (a tuple of INCONSISTENT) or of "triangle" -> (d [m, 8], cost, W)"""
    if key == "triangle":
        ent, rows, infos = triangle_case()
        w, anchor = weights(rows, INFO, infos), 1
    else:
        ent, rows, infos = inconsistent_case(*key)
        w, anchor = weights(rows, key[3], infos), 0
    d, cost = np_minimise(ent, rows, w, anchor)
    return d, cost, w


# ---- refused trials

# ring-8, seed 1, +-40 px, INFO weights.  From lambda0 = 1e-12 the host reference refuses 18 of 34 trials (the undamped steps overshoot until lambda has
# grown to where the default starts) and converges; at the default max_trials of 24 the same run ends at the cap.  From the default lambda0 = 1e-3 all 16
# trials are accepted: that run is the one the others are compared with.
REJECTING = ("ring-8", 1, 40.0, INFO)
REJECTING_KW = dict(weighting=INFO, lambda0=1e-12, max_trials=64)
REJECTING_TRIALS = (34, 16)
LAMBDA0S = (1e-12, 1e6, 1e100)
# two runs that each stop at a proposed step below eps_px (1e-6 px, the default) lie within eps_px of the minimum each, whatever their lambda0
LAMBDA0_GATE = 2e-6


def rejecting_case():
    return inconsistent_case(*REJECTING)


# ---- far maps

def far_shift(t):
    return R.shift(t, 0.5 * t)


@functools.lru_cache(maxsize=None)
def far_case(name, seed, t):
    """exact_case(name, seed) with every matrix right-multiplied by one shift of (t, t / 2) px: the relatives are the near case's in exact arithmetic
    -> (truths, entries, rows)"""
    truths, ent, ed = A.exact_case(name, seed)
    s = far_shift(t)
    e = np.array(ent)
    for k in range(len(e)):
        h = np.asarray(ent[k]["h_origin_key"], np.float64) @ s
        e[k]["h_origin_key"] = h / h[2, 2]
    e.setflags(write=False)
    return [x @ s for x in truths], e, ed


def far_error(hs, truths_near, t, mask=None):
    """the worst corner error of far matrices against the truth: the shift is taken off exactly (its inverse is a shift) before the near truth is"""
    back = far_shift(-t)
    return A.worst_error([np.asarray(h, np.float64).reshape(3, 3) @ back for h in hs], truths_near, mask)


# ---- the singular exits: name -> (entries, rows, infos, option fields)

def singular_cases():
    truths, ent, ed = A.exact_case("all-3", 0)
    out = {}
    # the undamped factorisation on entry: a free node whose only edge weighs nothing (keyframe_adjust_util.verdict_cases has it too)
    infos = np.tile(np.eye(8).reshape(64), (len(ed), 1))
    infos[1] = 0.0
    cut = np.array(ed)
    cut["flags"][2] = LOW_OVERLAP
    out["undamped pivot"] = (ent, cut, infos, dict(weighting=INFO))
    # the pivot bound is not finite: weights so large that a diagonal entry of A overflows while the cost (residuals of 1e-2 px and less) does not
    big = np.tile((np.eye(8) * 1.7e308).reshape(64), (len(ed), 1))
    out["pivot bound not finite"] = (ent, near_rows(ent, ed), big, dict(weighting=INFO))
    # the damped factorisation after the undamped one passed: lambda x A overflows (lambda0 = 1e100 is a valid option, weights of 1e250)
    huge = np.tile((np.eye(8) * 1e250).reshape(64), (len(ed), 1))
    out["damped pivot overflows"] = (ent, ed, huge, dict(weighting=INFO, lambda0=1e100))
    return out


def near_rows(ent, ed, off=0.01):
    """the rows of `ed` with residuals that are tiny at the start but not zero: the entries' own relatives, `off` px away in every component"""
    rows = np.array(ed)
    x = [np.asarray(k["h_origin_key"], np.float64) for k in ent]
    for q in range(len(rows)):
        rows["offsets_px"][q] = (K.corners(x[int(rows["j"][q])] @ np.linalg.inv(x[int(rows["i"][q])])) + off).astype(np.float32)
    return rows


# ---- index maps: every shape of node_of / unknown_of

@functools.lru_cache(maxsize=None)
def index_cases():
    """for m = 2 .. 8: the anchor at slot 0, in the middle and at the end (by links); an invalid entry between usable ones; an entry that only rejected
    edges reach between adjusted ones.  Edges within 0.5 px of the truth, so the minimum depends on the weights -> {name: (entries, rows, infos,
    option fields, the anchor, adjusted_mask and unconnected_mask expected)}"""
    out = {}
    for m in range(2, 9):
        rng = np.random.default_rng(300 + m)
        truths = [K.homography(rng.uniform(-40.0, 40.0, 8)) for _ in range(m)]
        hs = [K.homography(rng.uniform(-2.0, 2.0, 8)) @ t for t in truths]
        hs = [h / h[2, 2] for h in hs]
        prs = A.all_pairs(m) if m <= 3 or m % 2 else A.ring(m)
        offs = [(K.corners(truths[j] @ np.linalg.inv(truths[i])) + rng.uniform(-0.5, 0.5, 8)).astype(np.float32) for i, j in prs]
        rows = A.edge_rows(prs, offs)
        rows["mse"] = rng.uniform(0.2, 30.0, len(prs))
        weighting = INFO if m % 2 else UNIT
        infos = infos_spd(len(prs), m) if weighting == INFO else None
        kw = dict(weighting=weighting)
        full = (1 << m) - 1
        for a in sorted({0, m // 2, m - 1}):
            links = [1] * m
            links[a] = 0
            out["m=%d anchor %d" % (m, a)] = (R.entries(hs, links=links), rows, infos, kw, a, full, 0)
        if m >= 3:
            u = m // 2
            for a in (0, m - 1):
                links = [1] * m
                links[a] = 0
                links[u] = -5                                                # (the fewest links, and not usable: never the anchor)
                valid = [1] * m
                valid[u] = 0
                out["m=%d invalid %d anchor %d" % (m, u, a)] = (R.entries(hs, links=links, valid=valid), rows, infos, kw, a, full & ~(1 << u), 0)
            cut = np.array(rows)
            for q, p in enumerate(prs):
                if u in p:
                    cut["flags"][q] = LOW_OVERLAP
            links = [1] * m
            links[m - 1] = 0
            out["m=%d unconnected %d anchor %d" % (m, u, m - 1)] = (R.entries(hs, links=links), cut, infos, kw, m - 1, full & ~(1 << u), 1 << u)
    return out


# ---- hostile tables: the generator of the stand-alone driver of tests/cpp/keyframe_adjust_ref.cpp, restated

_MASK = (1 << 64) - 1


class _Lcg:
    def __init__(self, seed):
        self.s = seed & _MASK

    def next(self):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & _MASK
        return self.s

    def unit(self):
        return (self.next() >> 11) / 9007199254740992.0

    def hostile(self, scale):
        k = self.next() >> 60
        if k < 5:
            return (np.nan, np.inf, -np.inf, 1e300, 0.0)[k]
        return (self.unit() - 0.5) * scale


def _pair_slots(p, m):
    prs = A.all_pairs(m)
    return prs[p] if 0 <= p < len(prs) else None


HOSTILE_SEED, HOSTILE_TABLES = 12, 64                                        # (the seed: tests/test_keyframe_adjust_hostile_cpu.py says what it must give)


@functools.lru_cache(maxsize=None)
def hostile_tables(seed=HOSTILE_SEED, count=HOSTILE_TABLES):
    """-> [(entries [m], rows [n], infos [n, 64] or None, option fields)]: every third table wild - NaN, +-inf, 1e300 and 0 in entries, offsets, mse
    and information at the driver's rates, rows that point outside the table or have i >= j -, a quarter of the rows rejected, m in 1 .. 8, 0 .. 28
    rows, both weightings, apply 0 and 1, max_trials 1 .. 12, max_shift_px 0 or 5, a quarter of the tables without matrices"""
    g = _Lcg(seed)
    out = []
    for rnd in range(count):
        m = 1 + (g.next() >> 61)
        wild = rnd % 3 == 0
        ent = np.zeros(m, A.ENTRY)
        for k in range(m):
            ent[k]["valid"] = int((g.next() >> 62) != 0)
            ent[k]["links"] = g.next() >> 60
            ent[k]["serial"] = k + 1
            h = np.zeros(9)
            for c in range(9):
                ident = 1.0 if (c & 3) == 0 else 0.0
                sc = 60.0 if c in (2, 5) else 1e-5 if c in (6, 7) else 0.05
                h[c] = ident + (g.hostile(1e3) if wild and (g.next() >> 61) == 0 else (g.unit() - 0.5) * sc)
            if not wild:
                h[8] = 1.0
            ent[k]["h_origin_key"] = h.reshape(3, 3)
        n = g.next() % 29
        rows, infos = np.zeros(n, A.EDGE), np.zeros((n, 64))
        for q in range(n):
            p = _pair_slots(g.next() % 28, m)
            if p is None or (wild and (g.next() >> 61) == 0):
                p = ((g.next() >> 59) - 8, (g.next() >> 59) - 8)
            rows[q]["i"], rows[q]["j"] = p
            rows[q]["flags"] = LOW_OVERLAP if (g.next() >> 62) == 0 else ACCEPTED
            rows[q]["mse"] = g.hostile(50.0) if wild else g.unit() * 20.0
            with np.errstate(over="ignore"):
                for k in range(8):
                    rows[q]["offsets_px"][k] = np.float32(g.hostile(1e4) if wild and (g.next() >> 61) == 0 else (g.unit() - 0.5) * 80.0)
            for k in range(64):
                ident = 1e4 * g.unit() if k % 9 == 0 else 0.0
                infos[q, k] = g.hostile(1e5) if wild and (g.next() >> 60) == 0 else ident
        kw = dict(weighting=g.next() >> 63, apply=g.next() >> 63, max_trials=1 + g.next() % 12, max_shift_px=5.0 if g.next() >> 63 else 0.0)
        none = (g.next() >> 62) == 0
        g.next()                                                             # (the driver's cur_slot and min_grid, which are not part of a table)
        g.next()
        out.append((ent, rows, None if none else infos, kw))
    return out


def check_invariants(before, rec, kw, after=None):
    """the driver's invariants on a record (and, where the entries after the call are at hand, on them): no written matrix is non-finite, what is not
    adjusted keeps its bytes, the bookkeeping stays"""
    r = rec.reshape(-1)[0]
    adjusted = bool(int(r["flags"]) & ADJUSTED)
    for k in range(len(before)):
        in_set = adjusted and (int(r["adjusted_mask"]) >> k) & 1
        if in_set:
            assert np.isfinite(r["h_origin_key"][k]).all(), k
        else:
            assert r["h_origin_key"][k].tobytes() == before[k]["h_origin_key"].tobytes(), k
        if after is not None:
            moved = in_set and kw.get("apply", 0) and k != int(r["anchor"])
            if moved:
                assert np.isfinite(after[k]["h_origin_key"]).all() and after[k]["h_origin_key"].tobytes() == r["h_origin_key"][k].tobytes(), k
            else:
                assert after[k].tobytes() == before[k].tobytes(), k
            for f in ("valid", "links", "serial", "pad"):
                assert after[k][f] == before[k][f], (k, f)
    assert not r["h_origin_key"][len(before):].any()


# ---- two records compared

SOFT_FIELDS, SOFT_EDGE_FIELDS = ("cost0", "cost", "lambda"), ("r0_px", "r_px", "mse")


def same_record(dev, ref, what):
    """integers, masks, matrices, delta_px and the rows' tables by bytes; cost0, cost, lambda and the rows' r0_px, r_px and mse by bytes except that two
    NaNs are equal (an invalid operation gives a NaN of the other sign on x86 than on the GPU) -> the number of values that needed the exception"""
    d, r = dev.reshape(-1)[0], ref.reshape(-1)[0]
    bad, nans = [], 0

    def soft(a, b, name):
        nonlocal nans
        a, b = np.atleast_1d(a), np.atleast_1d(b)
        for x, y in zip(a, b):
            if x.tobytes() == y.tobytes():
                continue
            if np.isnan(x) and np.isnan(y):
                nans += 1
            else:
                bad.append((name, float(x), float(y)))

    for f in A.REC.names:
        if f == "edge":
            for g in A.EDGE.names:
                if g in SOFT_EDGE_FIELDS:
                    soft(d["edge"][g], r["edge"][g], "edge." + g)
                elif np.ascontiguousarray(d["edge"][g]).tobytes() != np.ascontiguousarray(r["edge"][g]).tobytes():
                    bad.append("edge." + g)
        elif f in SOFT_FIELDS:
            soft(d[f], r[f], f)
        elif np.asarray(d[f]).tobytes() != np.asarray(r[f]).tobytes():
            bad.append(f)
    if bad:
        raise AssertionError((what, bad, int(d["flags"]), int(r["flags"]), int(d["trials"]), int(r["trials"]), float(d["cost"]), float(r["cost"])))
    return nans


# ---- every input of the CPU tests that the device repeats: group -> {name: (entries, rows, infos, option fields)}

def part_a_cases():
    out = {"inconsistent": {}, "triangle": {}, "rejecting": {}, "far": {}, "singular": singular_cases()}
    for key in INCONSISTENT:
        ent, rows, infos = inconsistent_case(*key)
        out["inconsistent"][key] = (ent, rows, infos, dict(weighting=key[3], **TIGHT))
    out["triangle"]["triangle"] = triangle_case() + (dict(weighting=INFO, **TIGHT),)
    ent, rows, infos = rejecting_case()
    out["rejecting"]["refused trials"] = (ent, rows, infos, REJECTING_KW)
    out["rejecting"]["the trial cap"] = (ent, rows, infos, dict(REJECTING_KW, max_trials=24))
    out["rejecting"]["lambda0 1e-3"] = (ent, rows, infos, dict(REJECTING_KW, lambda0=1e-3))
    for l0 in LAMBDA0S[1:]:
        out["rejecting"]["lambda0 %g" % l0] = (ent, rows, infos, dict(REJECTING_KW, lambda0=l0))
    for name in ("all-8", "ring-8"):
        for seed in A.SEEDS:
            for t in (0.0,) + FAR_SHIFTS:
                truths, e, ed = far_case(name, seed, t) if t else A.exact_case(name, seed)
                out["far"][(name, seed, t)] = (e, ed, None, dict(weighting=UNIT))
    return out
