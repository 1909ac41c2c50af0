"""The solve of the joint adjustment on the device where it leaves the straight path (include/hnet.h hnet_op_keyframe_adjust_solve,
hnet_sessions_keyframe_adjust; csrc/kernels_keyframe_adjust.hip): every input of tests/test_keyframe_adjust_hostile_cpu.py - inconsistent
edges in both weightings, the asymmetric triangle, the run whose trials are refused (lanes read need_lin and A across iterations without rewriting them,
the factorisation runs again on an unchanged matrix, delta is kept when a trial is refused), the trial cap, each singular exit that can be reached, far
maps -, every shape of the index maps for m = 2 .. 8, 64 hostile tables and eight sessions in one call.  Each record is compared with the host
reference's by keyframe_adjust_hostile.same_record, and on the inconsistent edges delta_px also with the independent float64 minimiser.  A context of
max_batch 8; every test is a handful of solves on tables of at most 8 entries and 28 rows."""
import numpy as np
import pytest

import keyframe_adjust_hostile as X
import keyframe_adjust_util as A
from cuahn_vio_amd import _capi
from keyframe_adjust_hostile import ADJUSTED, CONVERGED, NO_GAIN, SINGULAR

pytestmark = pytest.mark.gpu

CAP = 8


@pytest.fixture(scope="module")
def aref(tmp_path_factory):
    return A.build_ref(tmp_path_factory.mktemp("keyframe_adjust_ref_gpu_hostile"))


@pytest.fixture(scope="module")
def eng(blob):
    from cuahn_vio_amd.homography_net import HnetEngine
    e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=8)
    yield e
    e.close()


def _both(eng, aref, case, what, nans=0, **more):
    """the device's record and the host's of one case, compared -> (device record, host record); nans: how many values may be equal only as NaNs
    (None: any number, returned as a third value)"""
    ent, rows, infos, kw = case
    o = A.opts(aref, **dict(kw, **more))
    dev = eng.op_keyframe_adjust_solve(ent, rows, infos, **A.opts_kw(o))
    ref = A.ref_solve(aref, ent, rows, o, infos)[0]
    n = X.same_record(dev, ref, what)
    if nans is None:
        return dev[0], ref[0], n
    assert n == nans, (what, n)
    return dev[0], ref[0]


def _against_minimum(eng, aref, key, case, anchor):
    r, _ = _both(eng, aref, case, key)
    d, cost, _ = X.minimum(key)
    diff = float(np.abs(r["delta_px"][:len(case[0])] - d).max())
    print(key, "trials", int(r["trials"]), "accepted", int(r["accepted"]), "|delta - numpy| %.3e px (gate %.2e), cost rel %.1e" % (diff, X.MINIMUM_GATE, abs(r["cost"] - cost) / cost))
    assert int(r["flags"]) == ADJUSTED | CONVERGED and int(r["anchor"]) == anchor
    assert diff <= X.MINIMUM_GATE and abs(r["cost"] - cost) <= X.COST_RTOL * cost
    return int(r["trials"]) - int(r["accepted"])


@pytest.mark.parametrize("name", ("all-3", "all-8", "ring-8"))
def test_inconsistent_edges(eng, aref, name):
    """edges off by +-0.5 and +-5 px, two seeds, both weightings, eps_px = 1e-9: the record equals the host's by bytes, and delta_px is the minimiser of
    an independent float64 Gauss-Newton within the gate measured on the host (ten times 1.10e-7 px) - the comparison the byte equality cannot give.
    With eps_px this small the last trials of several cases are refused, so these runs also restore from a refused trial"""
    cases = X.part_a_cases()["inconsistent"]
    refused = sum(_against_minimum(eng, aref, key, cases[key], 0) for key in X.INCONSISTENT if key[0] == name)
    print(name, "refused trials over the cases:", refused)
    assert refused > 0


def test_asymmetric_triangle(eng, aref):
    _against_minimum(eng, aref, "triangle", X.part_a_cases()["triangle"]["triangle"], 1)


def test_refused_trials_and_the_trial_cap(eng, aref):
    """the run that refuses 18 of its 34 trials, the same run at the default cap of 24 trials, and the runs from lambda0 = 1e-3, 1e6 and 1e100: every
    record by bytes; the device's own record has accepted < trials, so the path cannot silently disappear"""
    cases = X.part_a_cases()["rejecting"]
    r, _ = _both(eng, aref, cases["refused trials"], "refused trials")
    print("trials", int(r["trials"]), "accepted", int(r["accepted"]), "lambda", r["lambda"])
    assert int(r["accepted"]) < int(r["trials"]) and (int(r["trials"]), int(r["accepted"])) == X.REJECTING_TRIALS and int(r["flags"]) == ADJUSTED | CONVERGED
    cap, _ = _both(eng, aref, cases["the trial cap"], "the trial cap")
    assert int(cap["trials"]) == 24 and int(cap["flags"]) == ADJUSTED and int(cap["accepted"]) < 24
    base, _ = _both(eng, aref, cases["lambda0 1e-3"], "lambda0 1e-3")
    far, _ = _both(eng, aref, cases["lambda0 1e+06"], "lambda0 1e6")
    assert np.abs(far["delta_px"] - base["delta_px"]).max() <= X.LAMBDA0_GATE and np.abs(r["delta_px"] - base["delta_px"]).max() <= X.LAMBDA0_GATE
    top, _ = _both(eng, aref, cases["lambda0 1e+100"], "lambda0 1e100")
    assert int(top["flags"]) == NO_GAIN | CONVERGED and int(top["trials"]) == 0
    # with apply the refused run writes what it reached, the same record
    again, _ = _both(eng, aref, cases["refused trials"], "refused trials, apply", apply=1)
    assert again.tobytes() == r.tobytes()


@pytest.mark.parametrize("case", list(X.singular_cases()))
def test_singular_exits(eng, aref, case):
    """the undamped pivot, the pivot bound that is not finite and the damped pivot that overflows: ADJ_SINGULAR without a trial, by bytes"""
    r, _ = _both(eng, aref, X.singular_cases()[case], case)
    assert int(r["flags"]) == SINGULAR and int(r["trials"]) == 0 and not r["delta_px"].any()


@pytest.mark.parametrize("name", ("all-8", "ring-8"))
def test_far_maps(eng, aref, name):
    """maps 1e5 and 1e6 px from the origin: by bytes the host's, and verdict, masks and delta_px (within the gate measured on the host) the near map's"""
    cases = X.part_a_cases()["far"]
    for seed in A.SEEDS:
        near, _ = _both(eng, aref, cases[(name, seed, 0.0)], (name, seed, "near"))
        truths = A.exact_case(name, seed)[0]
        for t in X.FAR_SHIFTS:
            far, _ = _both(eng, aref, cases[(name, seed, t)], (name, seed, t))
            for f in ("flags", "anchor", "n_edges", "adjusted_mask", "unconnected_mask", "trials", "accepted"):
                assert int(far[f]) == int(near[f]), f
            dd = float(np.abs(far["delta_px"] - near["delta_px"]).max())
            print(name, "seed", seed, "shift %g px: |delta far - near| %.3e px" % (t, dd))
            assert int(far["flags"]) == ADJUSTED | CONVERGED and dd <= X.FAR_GATE_FACTOR * X.FAR_DELTA_WORST[t]
            assert X.far_error(far["h_origin_key"], truths, t) <= 10 * 4.72e-6                               # tests/test_keyframe_adjust_cpu.py EXACT_GATE


@pytest.mark.parametrize("m", range(2, 9))
def test_index_maps(eng, aref, m):
    """the anchor at slot 0, in the middle and at the end, an invalid entry between usable ones, an entry that only rejected edges reach between
    adjusted ones - every shape of node_of / unknown_of, and with it every extent N of the solve's loops: by bytes the host's; the anchor and every
    entry outside adjusted_mask keep their matrix bytes and every other one moves; apply = 1 gives the record of apply = 0.  (The operator-level call
    returns no entries: what apply writes into them is the record's matrices, read here; the entries themselves are read back in
    test_eight_sessions_in_one_call and tests/test_gpu_sessions_keyframe_adjust.py, and on the host in tests/test_keyframe_adjust_hostile_cpu.py)"""
    n = 0
    for name, (ent, rows, infos, kw, anchor, amask, umask) in X.index_cases().items():
        if not name.startswith("m=%d " % m):
            continue
        n += 1
        r, _ = _both(eng, aref, (ent, rows, infos, kw), name)
        r1, _ = _both(eng, aref, (ent, rows, infos, kw), name + ", apply", apply=1)
        assert r1.tobytes() == r.tobytes(), name
        assert int(r["flags"]) == ADJUSTED | CONVERGED and (int(r["anchor"]), int(r["adjusted_mask"]), int(r["unconnected_mask"])) == (anchor, amask, umask), name
        for k in range(m):
            moved = bool((amask >> k) & 1 and k != anchor)
            assert (r["h_origin_key"][k].tobytes() != ent[k]["h_origin_key"].tobytes()) == moved and bool(r["delta_px"][k].any()) == moved, (name, k)
        X.check_invariants(ent, np.array([r]), kw)
    assert n == (2 if m == 2 else 6)


def test_hostile_tables(eng, aref):
    """64 tables of the generator of the reference's stand-alone driver (NaN, +-inf, 1e300 and 0 in entries, offsets, mse and information; rows outside
    the table; rejected rows; m = 1 .. 8; both weightings, apply 0 and 1, max_trials 1 .. 12): each record equals the host's, two NaNs counting as
    equal in cost0, cost, lambda, r0_px, r_px and mse (the count is printed), and the driver's invariants hold on the device's record: no matrix of
    an adjusted entry is non-finite, every other matrix is the entry's own bytes.  tests/test_keyframe_adjust_hostile_cpu.py shows that these tables
    reach the solve, ADJ_ADJUSTED, the non-finite stops and a NaN cost0 often enough"""
    nans = ran = adjusted = 0
    for k, (ent, rows, infos, kw) in enumerate(X.hostile_tables()):
        r, _, n = _both(eng, aref, (ent, rows, infos, kw), ("table", k), nans=None)
        nans += n
        X.check_invariants(ent, np.array([r]), kw)
        ran += not int(r["flags"]) & (_capi.ADJ_FEW_ENTRIES | _capi.ADJ_NO_EDGES)
        adjusted += bool(int(r["flags"]) & ADJUSTED)
    print("values equal only as NaNs:", nans, "; tables that reach the solve:", ran, "; ADJUSTED:", adjusted)
    assert ran >= 24 and adjusted >= 8


def _map(s, cam):
    entries, mstate = s.keyframe_map_info(cam)
    return np.stack([s.map_keyframe(cam, j) for j in range(CAP)]), entries, mstate


def test_eight_sessions_in_one_call(eng):
    """a sessions object of 8 cameras, each tracked over three frames (three batched track calls; two cameras on the diagonal path with 2 jobs, the
    others with 3: 22 jobs, three rounds at max_batch 8): one keyframe_adjust over all 8 ids in a scrambled order gives every session the record and
    the edge records it gets alone - the solve kernel's grid at its largest -, a second identical call the same bytes, and with apply the maps hold the
    records' matrices with everything else as it was"""
    from cuahn_vio_amd.homography_net import HnetSessions
    kw = dict(A.TEXTURE_OPTS)
    s = HnetSessions(eng, 8)
    try:
        s.enable_keyframes()
        s.enable_keyframe_map(CAP)
        s.enable_keyframe_adjust()
        cams = list(range(8))
        seqs = [A.path_frames(seed, A.DIAGONAL_PATH) if c in (2, 5) else A.path_frames(seed) for c, seed in enumerate((2, 4, 5, 7, 8, 9, 11, 13))]
        for i in range(3):
            s.push(cams, np.stack([q[0][i] for q in seqs]))
            s.keyframe_track(cams, np.stack([q[2][i] for q in seqs]), **A.TRACK_KW)
        alone = [s.keyframe_adjust([c], want_edge_records=True, **kw) for c in cams]
        jobs = [int(a[0][0]["n_jobs"]) for a in alone]
        print("jobs", jobs, "flags", [int(a[0][0]["flags"]) for a in alone], "trials", [int(a[0][0]["trials"]) for a in alone])
        assert jobs == [3, 3, 2, 3, 3, 2, 3, 3] and all(int(a[0][0]["flags"]) & ADJUSTED for a in alone)
        ids = [5, 0, 7, 2, 6, 1, 4, 3]
        rec, er = s.keyframe_adjust(ids, want_edge_records=True, **kw)
        for k, c in enumerate(ids):
            assert rec[k].tobytes() == alone[c][0][0].tobytes() and er[k].tobytes() == alone[c][1][0].tobytes(), c
        rec2, er2 = s.keyframe_adjust(ids, want_edge_records=True, **kw)
        assert rec2.tobytes() == rec.tobytes() and er2.tobytes() == er.tobytes()
        before = {c: _map(s, c) for c in cams}
        rec3 = s.keyframe_adjust(ids, apply=1, **kw)
        assert rec3.tobytes() == rec.tobytes()
        for k, c in enumerate(ids):
            images, ent, ms = before[c]
            images2, ent2, ms2 = _map(s, c)
            assert ent2["h_origin_key"].tobytes() == rec[k]["h_origin_key"].tobytes() and images2.tobytes() == images.tobytes() and ms2.tobytes() == ms.tobytes()
            for j in range(CAP):
                moved = bool((int(rec[k]["adjusted_mask"]) >> j) & 1 and j != int(rec[k]["anchor"]))
                assert (ent2[j].tobytes() != ent[j].tobytes()) == moved, (c, j)
            for f in ("valid", "links", "serial", "pad"):
                assert ent2[f].tobytes() == ent[f].tobytes(), (c, f)
    finally:
        s.close()
