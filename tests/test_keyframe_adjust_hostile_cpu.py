"""What the byte-for-byte tests of the joint adjustment cannot see, on the host (include/hnet_keyframe_adjust.h through tests/cpp/keyframe_adjust_ref.cpp;
DESIGN 7ad).  Host and device compile the same header, so a wrong rule passes them, and on consistent edges every descent direction ends at the same
point.  Here the header's minimum on INCONSISTENT edges is compared with a float64 Gauss-Newton written from the statement of the problem
(keyframe_adjust_hostile.np_minimise), jacobian_col with central differences of edge_residual, and every input that
tests/test_gpu_keyframe_adjust_hostile.py sends to the device is first proven, on the host reference alone, to take the path it is meant to take: refused
trials, the trial cap, each singular exit that can be reached, far maps, every shape of the index maps, and the hostile tables.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import keyframe_adjust_hostile as X
import keyframe_adjust_util as A
from cuahn_vio_amd import _capi
from keyframe_adjust_hostile import ADJUSTED, CONVERGED, INFO, NO_GAIN, SINGULAR, UNIT

EXACT_GATE = 10 * 4.72e-6                                                    # tests/test_keyframe_adjust_cpu.py: the exact-edge cases against the truth


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = A.build_ref(tmp_path_factory.mktemp("keyframe_adjust_ref_hostile"))
    so.keyframe_adjust_ref_edge_residual.restype = C.c_int
    return so


def _solve(lib, case, **more):
    ent, rows, infos, kw = case
    return A.ref_solve(lib, ent, rows, A.opts(lib, **dict(kw, **more)), infos)


def _against_minimum(lib, key, case, anchor):
    """-> |delta_px - np_minimise| (px) after the asserts on the verdict and the cost"""
    ent, rows, infos, kw = case
    r = _solve(lib, case)[0][0]
    d, cost, w = X.minimum(key)
    m = len(ent)
    at = X.np_cost(ent, rows, w, r["delta_px"][:m])                           # the statement's cost at the header's point
    diff = float(np.abs(r["delta_px"][:m] - d).max())
    print(key, "trials", int(r["trials"]), "accepted", int(r["accepted"]), "cost %.12g numpy's minimum %.12g (rel %.1e) numpy's cost at the header's point rel %.1e"
          % (r["cost"], cost, abs(r["cost"] - cost) / cost, abs(at - r["cost"]) / r["cost"]), "|delta - numpy| %.3e px (gate %.2e)" % (diff, X.MINIMUM_GATE))
    assert int(r["flags"]) == ADJUSTED | CONVERGED and int(r["anchor"]) == anchor and int(r["n_edges"]) == len(rows)
    assert abs(at - r["cost"]) <= X.COST_RTOL * r["cost"] and abs(cost - r["cost"]) <= X.COST_RTOL * r["cost"]
    assert not r["delta_px"][anchor].any() and not r["delta_px"][m:].any()
    assert diff <= X.MINIMUM_GATE
    return diff, int(r["trials"]) - int(r["accepted"])


@pytest.mark.parametrize("name", ("all-3", "all-8", "ring-8"))
def test_minimum_on_inconsistent_edges(lib, name):
    """edge offsets off by +-0.5 and +-5 px, two seeds, both weightings (INFO with matrices and mse of an alignment's size), eps_px = 1e-9 and 64 trials:
    ADJUSTED | CONVERGED, the header's cost equals the statement's cost in numpy at its point and numpy's minimum to 1e-9 relative, and delta_px is
    numpy's minimiser within ten times the worst figure over all cases (1.10e-7 px, ring-8 seed 0 +-0.5 px UNIT; the figures per case are printed and
    stand in DESIGN 7ad; the floor is the finite-difference reference's).  On these inputs the cost stays far from zero, so the point reached depends
    on every column of the Jacobian, on the order of the endpoints in the normal matrix and on W against W^T"""
    assert X.MINIMUM_GATE < 1e-4                                               # 7q's host / device margin: a worst figure above it would be a finding
    cases = X.part_a_cases()["inconsistent"]
    got = [_against_minimum(lib, key, cases[key], 0) for key in X.INCONSISTENT if key[0] == name]
    print(name, "worst |delta - numpy| %.3e px; refused trials over the cases: %d" % (max(g[0] for g in got), sum(g[1] for g in got)))
    assert sum(g[1] for g in got) > 0                                          # with eps_px this small some last trials are refused: the device test counts on it


def test_asymmetric_triangle(lib):
    """a triangle in which only edge (1, 2) contradicts, weighed diag(1, 2 .. 128), the anchor slot 1: the free endpoints are i of one edge and j of
    another, and the weight tells the components apart - what a symmetric graph with scalar weights hides"""
    _against_minimum(lib, "triangle", X.part_a_cases()["triangle"]["triangle"], 1)


def _residual(lib, g, di, dj, z):
    r = np.zeros(8)
    ok = lib.keyframe_adjust_ref_edge_residual(A._p(g), A._p(di), A._p(dj), A._p(z), A._p(r))
    return ok, r


def _column(lib, g, di, dj, which, comp):
    c = np.zeros(8)
    lib.keyframe_adjust_ref_jacobian_col(A._p(g), A._p(di), A._p(dj), which, comp, A._p(c))
    return c


def test_jacobian_against_central_differences(lib):
    """all 16 columns of jacobian_col against central differences of edge_residual, both through the reference's exports: at d_i = d_j = 0, at deltas
    of +-2 px and of +-40 px, for G the identity, a relative of exact_case and a G with a projective row of 1e-4.  Per G and point the step is the one
    that minimises the difference; step and difference are printed.  Relative to the column's largest entry the worst observed is JACOBIAN_WORST, the
    gate ten times it: a wrong sign or a swapped endpoint misses by order 1.  And the NaN contract: a G whose product has no corners gives a NaN column
    and a false edge_residual with every r NaN"""
    truths, ent, ed = A.exact_case("all-3", 0)
    rel = np.asarray(ent[2]["h_origin_key"]) @ np.linalg.inv(np.asarray(ent[0]["h_origin_key"]))
    proj = np.array([[1.0, 0.02, 12.0], [-0.03, 1.0, -7.0], [1e-4, -1e-4, 1.0]])
    rng = np.random.default_rng(11)
    z = rng.uniform(-5.0, 5.0, 8)
    worst = 0.0
    for gname, g in (("identity", np.eye(3)), ("a relative", np.ascontiguousarray(rel / rel[2, 2])), ("projective row 1e-4", proj)):
        for size in (0.0, 2.0, 40.0):
            di, dj = rng.uniform(-size, size, 8), rng.uniform(-size, size, 8)
            cols = np.stack([_column(lib, g, di, dj, c // 8, c % 8) for c in range(16)])
            assert np.isfinite(cols).all()
            best = None
            for step in (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6):
                err = 0.0
                for c in range(16):
                    pair = []
                    for s in (step, -step):
                        a, b = di.copy(), dj.copy()
                        (b if c // 8 else a)[c % 8] += s
                        ok, r = _residual(lib, g, a, b, z)
                        assert ok == 1
                        pair.append(r)
                    fd = (pair[0] - pair[1]) / (2.0 * step)
                    err = max(err, float(np.abs(fd - cols[c]).max() / np.abs(cols[c]).max()))
                best = (err, step) if best is None or err < best[0] else best
            print("G %s, deltas of +-%g px: step %g px, worst |central difference - jacobian_col| / |column| %.3e (gate %.2e)" % (gname, size, best[1], best[0], X.JACOBIAN_GATE))
            worst = max(worst, best[0])
            assert best[0] <= X.JACOBIAN_GATE
    print("worst of all %.3e" % worst)
    assert X.JACOBIAN_GATE < 1e-3                                              # and order 1 is a thousand gates away
    # no corners: a corner behind the camera
    behind = np.diag([1.0, 1.0, -1.0])
    zero = np.zeros(8)
    ok, r = _residual(lib, behind, zero, zero, z)
    assert ok == 0 and np.isnan(r).all()
    for c in range(16):
        assert np.isnan(_column(lib, behind, zero, zero, c // 8, c % 8)).all()
    ok, r = _residual(lib, np.eye(3), zero, np.full(8, np.nan), z)
    assert ok == 0 and np.isnan(r).all()


def test_refused_trials_and_the_trial_cap(lib):
    """what the device's cases rely on, on the host alone.  ring-8 seed 1 with +-40 px on the edges and INFO weights, from lambda0 = 1e-12: 18 of 34
    trials are refused (A is factorised again under a raised lambda without a new linearisation, P.delta stays when a trial is refused) and the run
    converges; at the default max_trials the same run ends AT the cap, without ADJ_CONVERGED.  From lambda0 = 1e-3 every trial is accepted, and from
    1e-12 and 1e6 the run reaches that run's point within 2 eps_px and its cost to 1e-9.  From lambda0 = 1e100 the verdict is ADJ_NO_GAIN |
    ADJ_CONVERGED with no trial: under that damping the first proposal, (A + 1e100 diag A)^-1 g, is below eps_px, a step that small is not tried, and
    the cost is still cost0 - the run of refusals the header warns of, taken to its end: CONVERGED alone does not mean adjusted"""
    cases = X.part_a_cases()["rejecting"]
    r = _solve(lib, cases["refused trials"])[0][0]
    print("lambda0 1e-12: trials", int(r["trials"]), "accepted", int(r["accepted"]), "lambda %.3g cost0 %.6g cost %.12g" % (r["lambda"], r["cost0"], r["cost"]))
    assert int(r["flags"]) == ADJUSTED | CONVERGED and (int(r["trials"]), int(r["accepted"])) == X.REJECTING_TRIALS and int(r["accepted"]) < int(r["trials"])
    cap = _solve(lib, cases["the trial cap"])[0][0]
    print("at the default max_trials: trials", int(cap["trials"]), "accepted", int(cap["accepted"]), "flags", int(cap["flags"]))
    assert A.opts(lib).max_trials == 24 and int(cap["trials"]) == 24 and int(cap["flags"]) == ADJUSTED and int(cap["accepted"]) < 24
    base = _solve(lib, cases["lambda0 1e-3"])[0][0]
    assert int(base["flags"]) == ADJUSTED | CONVERGED and int(base["trials"]) == int(base["accepted"])
    for name in ("refused trials", "lambda0 1e+06"):
        o = _solve(lib, cases[name])[0][0]
        diff = float(np.abs(o["delta_px"] - base["delta_px"]).max())
        print(name, "trials", int(o["trials"]), "accepted", int(o["accepted"]), "|delta - that from 1e-3| %.3e px, cost rel %.1e" % (diff, abs(o["cost"] - base["cost"]) / base["cost"]))
        assert int(o["flags"]) == ADJUSTED | CONVERGED and diff <= X.LAMBDA0_GATE and abs(o["cost"] - base["cost"]) <= 1e-9 * base["cost"]
    top = _solve(lib, cases["lambda0 1e+100"])[0][0]
    print("lambda0 1e100: flags", int(top["flags"]), "trials", int(top["trials"]), "lambda", top["lambda"])
    assert int(top["flags"]) == NO_GAIN | CONVERGED and int(top["trials"]) == 0 and top["cost"] == top["cost0"] == base["cost0"] and not top["delta_px"].any()
    assert top["lambda"] == 1e100


def test_singular_exits(lib):
    """solve() says ADJ_SINGULAR at four places.  Three are reached from a table, each with trials == 0:
    (1) the undamped factorisation after a linearisation - a free node whose only edge weighs nothing;
    (2) the pivot bound 1e-12 max diag(A) is not finite - weights of 1.7e308 make a diagonal entry of A infinite while residuals of 0.01 px keep
        the cost finite (the same table with weights of 1e250 adjusts, and numpy's sum of that entry overflows);
    (3) the damped factorisation after the undamped one passed - this needs an overflow, and lambda0 = 1e100 (valid) times A of 1e250 is one: the same
        table from lambda0 = 1e-3 adjusts, so the undamped pivots pass.
    Not reached, and not forced: (4) a proposal that is not finite after both factorisations passed.  The pivots then exceed 1e-12 max diag(A), g is
    finite whenever the cost is (an infinite W r makes r^T W r infinite or NaN, and such a point is never accepted), so dx could only overflow
    through g / pivot with both near the ends of the range, which (1) - (3) catch first on every table tried.  (1) after an accepted step - the
    later linearisations - is not reached either: an accepted point has finite residuals and the rank of A is the graph's"""
    cases = X.singular_cases()
    for name, case in cases.items():
        r = _solve(lib, case, apply=1)
        print(name, "flags", int(r[0][0]["flags"]), "trials", int(r[0][0]["trials"]), "cost0", r[0][0]["cost0"], "lambda", r[0][0]["lambda"])
        assert int(r[0][0]["flags"]) == SINGULAR and int(r[0][0]["trials"]) == 0 and np.isfinite(r[0][0]["cost0"]) and r[0][0]["cost0"] > 0.0
        assert r[1].tobytes() == np.ascontiguousarray(case[0]).tobytes() and not r[0][0]["delta_px"].any()
    # (2): the same table under weights that do not overflow adjusts; a diagonal entry of A overflows in numpy too
    ent, rows, infos, kw = cases["pivot bound not finite"]
    assert int(A.ref_solve(lib, ent, rows, A.opts(lib, **kw), infos * (1e250 / 1.7e308))[0][0]["flags"]) & ADJUSTED
    x = [np.asarray(k["h_origin_key"], np.float64) for k in ent]
    zero = np.zeros(8)
    with np.errstate(over="ignore"):
        diag = sum(float((_column(lib, np.ascontiguousarray(x[j] @ np.linalg.inv(x[i])), zero, zero, int(j == 2), 0) ** 2).sum()) * 1.7e308
                   for i, j in A.all_pairs(3) if 2 in (i, j))
    assert np.isinf(diag)
    # (3): the undamped pivots pass - from the default lambda0 the table adjusts
    ent, rows, infos, kw = cases["damped pivot overflows"]
    assert int(A.ref_solve(lib, ent, rows, A.opts(lib, **dict(kw, lambda0=1e-3)), infos)[0][0]["flags"]) & ADJUSTED


def test_far_maps(lib):
    """the entries of exact_case("all-8" | "ring-8", s) right-multiplied by one shift of 1e5 and of 1e6 px (the relatives are unchanged in exact
    arithmetic): verdict, masks and trials are the near case's, delta_px is the near case's within ten times the worst difference measured (1.04e-10
    px at 1e5 px, 9.13e-10 px at 1e6 px: the rounding of X_j X_i^-1, which grows with the shift), and the adjusted matrices chain back to the truth
    within EXACT_GATE unscaled - measured, the error against the truth at either shift equals the near case's in its first three digits"""
    cases = X.part_a_cases()["far"]
    worst = {t: [0.0, 0.0] for t in X.FAR_SHIFTS}
    for name in ("all-8", "ring-8"):
        for seed in A.SEEDS:
            truths = A.exact_case(name, seed)[0]
            near = _solve(lib, cases[(name, seed, 0.0)])[0][0]
            for t in X.FAR_SHIFTS:
                case = cases[(name, seed, t)]
                far = _solve(lib, case)[0][0]
                dd = float(np.abs(far["delta_px"] - near["delta_px"]).max())
                before, err = X.far_error(case[0]["h_origin_key"], truths, t), X.far_error(far["h_origin_key"], truths, t)
                print(name, "seed", seed, "shift %g px: |delta far - near| %.3e px, corner error against the truth before %.3f after %.3e px (near: %.3e)"
                      % (t, dd, before, err, A.worst_error(near["h_origin_key"], truths)))
                for f in ("flags", "anchor", "n_edges", "adjusted_mask", "unconnected_mask", "trials", "accepted"):
                    assert int(far[f]) == int(near[f]), f
                assert int(far["flags"]) == ADJUSTED | CONVERGED and int(far["adjusted_mask"]) == 255
                assert dd <= X.FAR_GATE_FACTOR * X.FAR_DELTA_WORST[t] and before > 1.0 and err <= EXACT_GATE
                worst[t] = [max(worst[t][0], dd), max(worst[t][1], err)]
    print("worst per shift (|delta far - near|, error against the truth):", worst)


@pytest.mark.parametrize("m", range(2, 9))
def test_index_maps(lib, m):
    """the anchor at slot 0, in the middle and at the end, an invalid entry between usable ones, an entry that only rejected edges reach between
    adjusted ones: the anchor and the masks are the expected ones, and with apply the entries are written exactly where adjusted_mask says (the anchor
    and everything outside keep their bytes), the record the same as without apply"""
    n = 0
    for name, (ent, rows, infos, kw, anchor, amask, umask) in X.index_cases().items():
        if not name.startswith("m=%d " % m):
            continue
        n += 1
        rec0, after0 = A.ref_solve(lib, ent, rows, A.opts(lib, **kw), infos)
        rec1, after1 = A.ref_solve(lib, ent, rows, A.opts(lib, apply=1, **kw), infos)
        r = rec1[0]
        assert int(r["flags"]) == ADJUSTED | CONVERGED, name
        assert (int(r["anchor"]), int(r["adjusted_mask"]), int(r["unconnected_mask"])) == (anchor, amask, umask), name
        assert rec0.tobytes() == rec1.tobytes() and after0.tobytes() == np.ascontiguousarray(ent).tobytes()
        for k in range(m):
            moved = (amask >> k) & 1 and k != anchor
            assert (after1[k].tobytes() != ent[k].tobytes()) == bool(moved), (name, k)
            assert r["h_origin_key"][k].tobytes() == after1[k]["h_origin_key"].tobytes() and bool(r["delta_px"][k].any()) == bool(moved)
        X.check_invariants(ent, rec1, dict(apply=1), after1)
    assert n == (2 if m == 2 else 6)


def test_hostile_tables_are_not_vacuous(lib):
    """the 64 tables of keyframe_adjust_hostile.hostile_tables (the generator of the reference's stand-alone driver restated, seed 12): the driver's
    invariants hold on the host, and the seed is one under which the tables do not pass vacuously: at least 24 reach the solve (neither FEW_ENTRIES
    nor NO_EDGES), at least 8 end ADJ_ADJUSTED, at least 3 end ADJ_SINGULAR or ADJ_NO_GAIN with a cost that is not finite, at least one has a NaN
    cost0; and every m in 1 .. 8, both weightings and both values of apply occur"""
    tables = X.hostile_tables()
    assert len(tables) == 64
    reach = adjusted = stopped = nan0 = 0
    for ent, rows, infos, kw in tables:
        rec, after = A.ref_solve(lib, ent, rows, A.opts(lib, **kw), infos)
        X.check_invariants(ent, rec, kw, after)
        r = rec[0]
        f = int(r["flags"])
        ran = not f & (_capi.ADJ_FEW_ENTRIES | _capi.ADJ_NO_EDGES)
        reach += ran
        adjusted += bool(f & ADJUSTED)
        stopped += bool(ran and f & (SINGULAR | NO_GAIN) and not np.isfinite(r["cost"]))
        nan0 += bool(np.isnan(r["cost0"]))
    print("of 64 tables: %d reach the solve, %d ADJUSTED, %d SINGULAR or NO_GAIN with a cost that is not finite, %d with a NaN cost0" % (reach, adjusted, stopped, nan0))
    assert reach >= 24 and adjusted >= 8 and stopped >= 3 and nan0 >= 1
    assert {len(t[0]) for t in tables} == set(range(1, 9)) and {t[3]["weighting"] for t in tables} == {UNIT, INFO} and {t[3]["apply"] for t in tables} == {0, 1}
    assert any(t[2] is None for t in tables) and max(len(t[1]) for t in tables) >= 24 and {t[3]["max_trials"] for t in tables} >= {1, 12}
