"""hnet_filters with a photometric gate (include/hnet.h hnet_filters_set_photo_gate; csrc/kernels_photo.hip photo_iter_kernel / photo_gate_kernel).
A gate that cannot reject must change nothing, bit for bit; the records of a gated step stay the operator call's; a rejection must skip exactly the
updates hnet_ekf::iterated_update_photo_gated names, show in both kinds of records and leave every other session alone; the NIS gate and a singular S
come first; the statistics count each judged record once, through a repeated attempt too.  8 sessions, max_batch 8, 12 images (reference gate open),
windows of 0 - 40 intervals, main model prior-3, N = 16.  "Ratio" is the host quotient (est.sum_inside / est.n_inside) / (prior.sum_inside /
prior.n_inside) of record [2 + it] to record [1]."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_filters as tg
import test_gpu_filters_innov as ti
import test_sessions_iterative_cpu as ic

pytestmark = pytest.mark.gpu

NPIX = 224 * 320
DEGENERATE, PH_REJECTED = 1, 2
NONE, USED, REJECTED, SINGULAR, SKIPPED = range(5)
INVALID = 1
PREC_BF16X3, PREC_F16X2 = 2, 3
COUNTS = [0, 1, 2, 16, 40, 16, 3, 7]
T_FRAME = 1.0 + 0.1 * 11
# Tests b - f share one set of inputs.  All 8 sessions see the same images; their ratios differ through their priors and grow by a few per cent from one
# iteration to the next in a session whose updates move it.  Test c needs 4 sessions that stay below a gate in every iteration, so (as test c of
# test_gpu_filters_innov.py does for the NIS) the sessions are two groups of cameras: LO_GROUP weighs the network covariance with K_LO times the default
# k_net_cov, its gain falls accordingly, its state and prior hardly move, and its ratio stays within the dropout noise of its first value.  The ratio of
# iteration 0 does not depend on k_net_cov, so the groups were read off an ungated run; every test asserts what it needs of them.
SEED, LO_GROUP, K_LO = 81, (3, 4, 5, 7), 1000.0

_OPEN = []


def _track(*objs):
    """objects to close if the test fails before its own close calls, the last one first: a filters object left to the garbage collector may be destroyed
    after its sessions and engine"""
    _OPEN.extend(objs)
    return objs


@pytest.fixture(autouse=True)
def _close_in_order():
    yield
    while _OPEN:
        _OPEN.pop().close()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return ti._build(tmp_path_factory.mktemp("filters_ref_pg"), "filters_ref")


@pytest.fixture(scope="module")
def pgref(tmp_path_factory):
    return ti._build(tmp_path_factory.mktemp("filters_photo_gate_ref_pg"), "filters_photo_gate_ref")


def _cands(priors, net):
    """the filters' candidates [n, 2 + iters, 8]: zero, the fp32 prior of iteration 0, the packed mean of every forward"""
    iters, n = net.shape[0], net.shape[1]
    return np.concatenate([np.zeros((n, 1, 8), np.float32), priors[0][:, None, :], np.transpose(net[:, :, :8], (1, 0, 2))], axis=1).reshape(n, 2 + iters, 8)


def _operator(e, s, f, ids, net):
    prev, curr = np.stack([s.frame(int(i), 0) for i in ids]), np.stack([s.frame(int(i), 1) for i in ids])
    return e.op_photo_residual(prev, curr, _cands(f.last_priors(len(ids)), net))


def _unflag(rec):
    r = rec.copy()
    r["flags"] &= ~PH_REJECTED
    return r


def _ratios(rec):
    """[n, iters]: record [2 + it] against record [1]"""
    pr = rec["sum_inside"][:, 1] / rec["n_inside"][:, 1]
    return (rec["sum_inside"][:, 2:] / rec["n_inside"][:, 2:]) / pr[:, None]


def _first_over(ratios, gate):
    """the iteration at which a session with these ungated ratios is refused by `gate`, or None (until then a gated step is the ungated one)"""
    hit = np.flatnonzero(np.asarray(ratios) > gate)
    return int(hit[0]) if len(hit) else None


def _want_stats(rec, upd, innov=None, open_gate=True):
    """hnet_photo_stats of one session from its records [2 + iters] of one call, as include/hnet.h defines them"""
    st = {"judged": 0, "rejected": 0, "degenerate": 0, "sum_ratio": 0.0, "max_ratio": 0.0}
    if not open_gate:
        return st
    pr = rec[1]
    for it in range(len(rec) - 2):
        e = rec[2 + it]
        st["judged"] += 1
        st["rejected"] += int(bool(e["flags"] & PH_REJECTED))
        st["degenerate"] += int(bool(e["flags"] & DEGENERATE))
        if not ((pr["flags"] | e["flags"]) & DEGENERATE) and pr["n_inside"] >= 1 and e["n_inside"] >= 1:
            r = (e["sum_inside"] / e["n_inside"]) / (pr["sum_inside"] / pr["n_inside"])
            if np.isfinite(r):
                st["sum_ratio"] += float(r)
                st["max_ratio"] = max(st["max_ratio"], float(r))
        stop = bool(e["flags"] & PH_REJECTED) or (upd < 0 and -1 - upd == it)
        if innov is not None:
            stop = stop or innov["flag"][it] in (REJECTED, SINGULAR)
        if stop:
            break
    return st


def _check_stats(f, ids, calls):
    """photo_stats of every listed session equals the count over its records of all `calls` [(rec, upd, innov or None)]; reset zeroes them"""
    for k, i in enumerate(ids):
        want = {"judged": 0, "rejected": 0, "degenerate": 0, "sum_ratio": 0.0, "max_ratio": 0.0}
        for rec, upd, innov in calls:
            one = _want_stats(rec[k], int(upd[k]), None if innov is None else innov[:, k])
            for key in ("judged", "rejected", "degenerate"):
                want[key] += one[key]
            want["sum_ratio"] += one["sum_ratio"]
            want["max_ratio"] = max(want["max_ratio"], one["max_ratio"])
        got = f.photo_stats(int(i))
        assert (got["judged"], got["rejected"], got["degenerate"]) == (want["judged"], want["rejected"], want["degenerate"]), (i, got, want)
        assert got["sum_ratio"] == pytest.approx(want["sum_ratio"], rel=1e-12, abs=0.0) and got["max_ratio"] == want["max_ratio"], (i, got, want)
        f.reset_photo_stats(int(i))
        assert f.photo_stats(int(i)) == {"judged": 0, "rejected": 0, "degenerate": 0, "sum_ratio": 0.0, "max_ratio": 0.0}


def _fleet(blob, iters, innov, frames=12, **kw):
    e, s, f = _track(*tg._setup(blob, 8, iters, frames=frames, **kw))
    if innov:
        f.enable_innovations()
    f.enable_photometric()
    return e, s, f


def _everything(f, s, ids, got, innov):
    n = len(ids)
    return [x.tobytes() for x in got] + [f.last_priors(n).tobytes(), f.get_state(ids).tobytes(), f.last_photometric(n).tobytes(),
                                         f.last_innovations(n).tobytes() if innov else b"", repr([s.seq(int(i)) for i in ids]).encode()]


@pytest.mark.parametrize("innov", [False, True])
@pytest.mark.parametrize("iters", [1, 3])
def test_gate_that_cannot_reject_changes_nothing_step(blob, iters, innov):
    """a. max_ratio = 1e30 on all 8 sessions: states, net_out, priors, updates, sequence numbers, innovation records and photometric records are those of an
    object with records on and no gate, byte for byte; the records come from the per-iteration launches in one object and the one launch in the other"""
    _capi, _, _, HnetFilters = tg._mods()
    ea, sa, fa = _fleet(blob, iters, innov)
    eb, sb, fb = _fleet(blob, iters, innov)
    ids = np.arange(8, dtype=np.int32)
    for i in ids:
        fa.set_photo_gate(int(i), 1e30)
    ps, sts, imus = ti._inputs(_capi, HnetFilters, 90 + iters, 8, T_FRAME, COUNTS)
    for f, s in ((fa, sa), (fb, sb)):
        ti._load(f, s, ps, sts, seq=7)
    a, b = fa.step(ids, [T_FRAME] * 8, imus), fb.step(ids, [T_FRAME] * 8, imus)
    assert _everything(fa, sa, ids, a, innov) == _everything(fb, sb, ids, b, innov)
    rec = fa.last_photometric(8)
    assert list(a[2]) == [iters] * 8 and not rec["flags"].any() and [sa.seq(int(i)) for i in ids] == [7 + iters] * 8
    assert rec.tobytes() == _operator(ea, sa, fa, ids, a[1]).tobytes()
    inn = fa.last_innovations(8) if innov else None
    for f, got in ((fa, a), (fb, b)):                                         # the statistics are kept for gated and ungated sessions alike
        _check_stats(f, ids, [(rec, got[2], inn)])
    for o in (fa, fb, sa, sb, ea, eb):
        o.close()


@pytest.mark.parametrize("innov", [False, True])
def test_gate_that_cannot_reject_changes_nothing_advance(blob, innov):
    """a. the same for three hnet_filters_advance ticks on rings of 64 readings that wrap (the set-up of test_gpu_filters_innov's test_off_is_off_advance)"""
    _capi, _, _, HnetFilters = tg._mods()
    iters = 3
    ea, sa, fa = _fleet(blob, iters, innov)
    eb, sb, fb = _fleet(blob, iters, innov)
    fa.enable_feed(64)
    fb.enable_feed(64)
    rng = np.random.default_rng(23)
    ids = np.arange(8, dtype=np.int32)
    t_frame = np.full(8, T_FRAME)
    ps, hist, fed = [], [], [0] * 8
    for i in range(8):
        p = tg._params(HnetFilters, rng, i)
        st = tg._state(_capi, rng, t_frame[i])
        for f in (fa, fb):
            f.set_params(i, p)
            f.set_state(i, st)
        fa.set_photo_gate(i, 1e30)
        ps.append(p)
        ts = t_frame[i] + p.cam_imu_dt - 0.0007 + 0.002 * np.arange(3 * 42 + 4)
        r = np.zeros(len(ts), _capi.IMU_DTYPE)
        r["t"], r["wm"], r["am"] = ts, rng.standard_normal((len(ts), 3)) * 0.3, rng.standard_normal((len(ts), 3)) * 0.5 + [0, 0, 9.81]
        hist.append(r)
    fr = tg._frames(rng, 3)
    calls = []
    for tick in range(3):
        t_frame = t_frame + 0.002 * np.maximum(COUNTS, 0.1) + 0.0004
        for s in (sa, sb):
            s.push(ids, np.repeat(fr[tick][None], 8, 0), t=list(t_frame))
        chunks = []
        for i in range(8):
            upto = int(np.searchsorted(hist[i]["t"], t_frame[i] + ps[i].cam_imu_dt, side="right")) + 1
            chunks.append(hist[i][fed[i]:upto])
            fed[i] = upto
        for f in (fa, fb):
            f.feed_imu(ids, chunks)
        a, b = fa.advance(ids), fb.advance(ids)
        assert list(a[3]) == [_capi.ADV_STEPPED] * 8 and list(a[2]) == [iters] * 8
        assert _everything(fa, sa, ids, a, innov) == _everything(fb, sb, ids, b, innov), tick
        rec = fa.last_photometric(8)
        assert not rec["flags"].any()
        calls.append((rec, a[2], fa.last_innovations(8) if innov else None))
    assert max(fed) > 64                                                      # the rings wrapped
    for f in (fa, fb):
        _check_stats(f, ids, calls)
    for o in (fa, fb, sa, sb, ea, eb):
        o.close()


def _ungated(blob, innov, iters=3):
    """a fleet with records on, the shared inputs and its ungated step: (e, s, f), (ps, sts, imus), ids, step result, records, ratios [8, iters]"""
    _capi, _, _, HnetFilters = tg._mods()
    e, s, f = _fleet(blob, iters, innov)
    ps, sts, imus = ti._inputs(_capi, HnetFilters, SEED, 8, T_FRAME, COUNTS)
    for i in LO_GROUP:
        ps[i].k_net_cov *= K_LO
    ids = np.arange(8, dtype=np.int32)
    ti._load(f, s, ps, sts, seq=4)
    ung = f.step(ids, [T_FRAME] * 8, imus)
    rec = f.last_photometric(8)
    assert list(ung[2]) == [iters] * 8 and not rec["flags"].any() and np.all(rec["n_inside"][:, 1:] >= 1)
    return (e, s, f), (ps, sts, imus), ids, ung, rec, _ratios(rec)


def test_records_stay_the_operators_and_tap_forms_agree(blob):
    """b. a gated step with rejections at several iterations: every record, the REJECTED bit aside, equals hnet_op_photo_residual on
    [0, last_priors[0], net_out[it][:, :8]] byte for byte, with the single-candidate launches reading img2 through LDS and from global memory alike"""
    (e, s, f), (ps, sts, imus), ids, ung, rec_u, ratio = _ungated(blob, innov=False)
    gates = [0.5 * (ratio[i].min() + ratio[i].max()) for i in range(8)]
    want_at = [_first_over(ratio[i], gates[i]) for i in range(8)]
    assert sum(w is not None for w in want_at) >= 4 and len({w for w in want_at if w is not None}) >= 2, (ratio, want_at)
    for i in ids:
        f.set_photo_gate(int(i), gates[i])
    got = {}
    for taps in (False, True):
        f.set_photo_gate_taps(taps)
        ti._load(f, s, ps, sts, seq=4)
        out, net, upd = f.step(ids, [T_FRAME] * 8, imus)
        rec = f.last_photometric(8)
        assert _unflag(rec).tobytes() == _operator(e, s, f, ids, net).tobytes(), taps
        for i in range(8):
            w = want_at[i]
            assert list(rec["flags"][i]) == [0, 0] + [PH_REJECTED if it == w else 0 for it in range(3)], (i, w, rec["flags"][i])
            assert upd[i] == (3 if w is None else w)
        got[taps] = [out.tobytes(), net.tobytes(), upd.tobytes(), rec.tobytes()]
    assert got[False] == got[True]
    for o in (f, s, e):
        o.close()


def test_rejection_at_iteration_zero(blob):
    """c. the gate at the midpoint between the 4th and 5th largest iteration-0 ratio of 8 sessions: the 4 above are refused at once and end where a step
    with the reference gate closed ends (propagation + reset), the 4 below are untouched; every forward still runs; the statistics follow the records"""
    (e, s, f), (ps, sts, imus), ids, ung, rec_u, ratio = _ungated(blob, innov=True)
    ec, sc, fc = _track(*tg._setup(blob, 8, 3, frames=6))                     # 6 images: the reference gate stays closed
    inn_u = f.last_innovations(8)
    order = np.sort(ratio[:, 0])[::-1]
    assert order[3] != order[4], order
    gate = 0.5 * (order[3] + order[4])
    above = ratio[:, 0] > gate
    print(f"iteration-0 ratios {np.array2string(ratio[:, 0], precision=5)}, gate {gate:.6g}; later {np.array2string(ratio[:, 1:].T, precision=5)}")
    assert above.sum() == 4 and sorted(np.flatnonzero(~above)) == list(LO_GROUP)
    assert ratio[~above].max() < gate, "the 4 below must stay below in iterations 1 and 2, or the rule refuses them later"
    for i in ids:
        f.set_photo_gate(int(i), gate)
    ti._load(f, s, ps, sts, seq=4)
    ti._load(fc, sc, ps, sts, seq=4)
    got = f.step(ids, [T_FRAME] * 8, imus)
    rec_g, inn_g = f.last_photometric(8), f.last_innovations(8)
    closed = fc.step(ids, [T_FRAME] * 8, imus)
    assert list(closed[2]) == [0] * 8
    for i in range(8):
        if above[i]:
            assert list(rec_g["flags"][i]) == [0, 0, PH_REJECTED, 0, 0]
            assert list(inn_g["flag"][:, i]) == [SKIPPED] * 3 and not inn_g["nis"][:, i].any() and got[2][i] == 0
            assert got[0][i].tobytes() == closed[0][i].tobytes()
            assert _unflag(rec_g)[i, :3].tobytes() == rec_u[i, :3].tobytes()
        else:
            assert got[2][i] == 3 and got[0][i].tobytes() == ung[0][i].tobytes()
            assert rec_g[i].tobytes() == rec_u[i].tobytes() and inn_g[:, i].tobytes() == inn_u[:, i].tobytes()
    assert _unflag(rec_g).tobytes() == _operator(e, s, f, ids, got[1]).tobytes()
    assert got[1][0].tobytes() == ung[1][0].tobytes() and np.all(np.isfinite(got[1]))
    assert [s.seq(int(i)) for i in ids] == [4 + 3] * 8                        # the forwards ran for all 8
    assert f.get_state(ids).tobytes() == got[0].tobytes()
    _check_stats(f, ids, [(rec_u, ung[2], inn_u), (rec_g, got[2], inn_g)])
    assert [f.innovation_stats(int(i))["rejected"] for i in ids] == [0] * 8
    for o in (f, fc, s, sc, e, ec):
        o.close()


def test_rejection_at_a_later_iteration(blob, ref, pgref):
    """d. every session whose iteration-1 or iteration-2 ratio exceeds its iteration-0 ratio gets a gate between the two: updates = the rejecting
    iteration, REJECTED there only, innovation flags USED before and SKIPPED from it on, and the state is filters_ref's propagation followed by
    hnet_ekf::iterated_update_photo_gated (filters_photo_gate_ref) fed the step's own network outputs and records"""
    _capi = tg._mods()[0]
    (e, s, f), (ps, sts, imus), ids, ung, rec_u, ratio = _ungated(blob, innov=True)
    inn_u = f.last_innovations(8)
    later = ratio[:, 1:].max(axis=1)
    chosen = [i for i in range(8) if later[i] > ratio[i, 0] * (1 + 1e-9)]
    print(f"ratios per session {np.array2string(ratio, precision=6)}; chosen {chosen}")
    assert len(chosen) >= 2, ratio
    gates = {i: 0.5 * (ratio[i, 0] + later[i]) for i in chosen}
    for i, g in gates.items():
        f.set_photo_gate(i, g)
    ti._load(f, s, ps, sts, seq=4)
    out, net, upd = f.step(ids, [T_FRAME] * 8, imus)
    rec, inn = f.last_photometric(8), f.last_innovations(8)
    assert _unflag(rec).tobytes() == _operator(e, s, f, ids, net).tobytes()
    for i in range(8):
        if i not in gates:
            assert out[i].tobytes() == ung[0][i].tobytes() and upd[i] == 3 and rec[i].tobytes() == rec_u[i].tobytes()
            continue
        at = _first_over(ratio[i], gates[i])
        assert at in (1, 2) and upd[i] == at
        assert list(rec["flags"][i]) == [0, 0] + [PH_REJECTED if it == at else 0 for it in range(3)]
        assert list(inn["flag"][:, i]) == [USED] * at + [SKIPPED] * (3 - at)
        # the host loop, fed this step's outputs and records (the prior's, then one per forward)
        st = np.array(sts[i], dtype=_capi.FILTER_STATE_DTYPE).reshape(1).copy()
        r = np.ascontiguousarray(imus[i])
        assert ref.ref_propagate_with_imu(C.c_void_p(st.ctypes.data), C.byref(ps[i]), C.c_double(T_FRAME), C.c_void_p(r.ctypes.data), len(r)) >= 0
        nn = np.ascontiguousarray(net[:, i, :], dtype=np.float32)
        script = np.ascontiguousarray(_unflag(rec)[i, 1:])
        hin, hrec = np.zeros(3, _capi.INNOVATION_DTYPE), np.zeros(4, _capi.PHOTO_RESIDUAL_DTYPE)
        u = pgref.photo_gate_ref_iterated(C.c_void_p(st.ctypes.data), C.byref(ps[i]), 3, C.c_void_p(nn.ctypes.data), 1, C.c_double(0.0),
                                          C.c_void_p(script.ctypes.data), C.c_double(gates[i]), 0, C.c_void_p(hin.ctypes.data), C.c_void_p(hrec.ctypes.data),
                                          None, None, None)
        assert u == at and list(hin["flag"]) == list(inn["flag"][:, i]) and list(hrec["flags"]) == list(rec["flags"][i, 1:])
        tg._close(out[i], st[0])
        for fld in ("r", "s_diag", "nis"):
            assert ti._rel(inn[fld][:, i], hin[fld]) <= ti.TOL
    _check_stats(f, ids, [(rec_u, ung[2], inn_u), (rec, upd, inn)])
    for o in (f, s, e):
        o.close()


def test_both_gates_together(blob):
    """e. session A: a NIS gate that rejects at iteration 0 and a photometric gate that would refuse later - no PHOTO_REJECTED anywhere; session B: refused
    photometrically at iteration 0 under a NIS gate of 1e-300 - PHOTO_REJECTED, innovation records all SKIPPED, nothing counted as a NIS rejection"""
    (e, s, f), (ps, sts, imus), ids, ung, rec_u, ratio = _ungated(blob, innov=True)
    later = ratio[:, 1:].max(axis=1)
    chosen = [i for i in range(8) if later[i] > ratio[i, 0] * (1 + 1e-9)]
    assert len(chosen) >= 1
    A = chosen[0]
    B = next(i for i in range(8) if i != A)
    f.set_photo_gate(A, 0.5 * (ratio[A, 0] + later[A]))
    f.set_nis_gate(A, 1e-300)
    f.set_photo_gate(B, 0.5 * ratio[B, 0])
    f.set_nis_gate(B, 1e-300)
    for i in ids:
        f.reset_innovation_stats(int(i))
    ti._load(f, s, ps, sts, seq=4)
    out, net, upd = f.step(ids, [T_FRAME] * 8, imus)
    rec, inn = f.last_photometric(8), f.last_innovations(8)
    assert list(inn["flag"][:, A]) == [REJECTED, SKIPPED, SKIPPED] and not rec["flags"][A].any() and upd[A] == 0
    assert list(rec["flags"][B]) == [0, 0, PH_REJECTED, 0, 0] and list(inn["flag"][:, B]) == [SKIPPED] * 3 and upd[B] == 0
    assert f.innovation_stats(A)["rejected"] == 1 and f.innovation_stats(B)["rejected"] == 0
    assert _unflag(rec).tobytes() == _operator(e, s, f, ids, net).tobytes()
    for i in range(8):
        if i not in (A, B):
            assert out[i].tobytes() == ung[0][i].tobytes() and upd[i] == 3
    f.reset_photo_stats(A), f.reset_photo_stats(B)
    for o in (f, s, e):
        o.close()


def test_min_inside_and_a_gate_that_only_counts_pixels(blob):
    """f. a gate of min_inside = 71 680 refuses an estimate that loses any pixel, whatever its ratio; the same session with min_inside = 0 and
    max_ratio = 1e30 is not refused"""
    (e, s, f), (ps, sts, imus), ids, ung, rec_u, ratio = _ungated(blob, innov=False)
    lose = [i for i in range(8) if rec_u["n_inside"][i, 2] < NPIX]
    assert lose, rec_u["n_inside"][:, 2]
    i = lose[0]
    f.set_photo_gate(i, 1e30, min_inside=NPIX)
    ti._load(f, s, ps, sts, seq=4)
    out, net, upd = f.step(ids, [T_FRAME] * 8, imus)
    rec = f.last_photometric(8)
    assert list(rec["flags"][i]) == [0, 0, PH_REJECTED, 0, 0] and upd[i] == 0 and rec["n_inside"][i, 2] < NPIX
    assert all(upd[k] == 3 and rec[k].tobytes() == rec_u[k].tobytes() and out[k].tobytes() == ung[0][k].tobytes() for k in range(8) if k != i)
    f.set_photo_gate(i, 1e30, min_inside=0)
    ti._load(f, s, ps, sts, seq=4)
    out, net, upd = f.step(ids, [T_FRAME] * 8, imus)
    assert upd[i] == 3 and f.last_photometric(8).tobytes() == rec_u.tobytes() and out.tobytes() == ung[0].tobytes()
    for o in (f, s, e):
        o.close()


def test_repeat_counts_once(blob):
    """g. the overflowing iterative model of test_gpu_filters_innov's test_repair_counts_once with gates set: the step demotes the model once and reruns;
    records, verdicts and statistics are those of fresh objects whose iterative engine runs HNET_PREC_BF16X3 from the start, each record counted once.
    The gates come from an ungated BF16X3 step: per session the midpoint of its smallest and largest ratio."""
    from cuahn_vio_amd.homography_net import HnetEngine
    _capi, _, _, HnetFilters = tg._mods()
    iters, n = 3, 4
    ov = ic.overflow_iterative_blob()
    ps, sts, imus = ti._inputs(_capi, HnetFilters, 47, n, T_FRAME, [16])
    ids = np.arange(n, dtype=np.int32)
    res, gates = [], None
    for prec in (PREC_BF16X3, PREC_F16X2, PREC_BF16X3):
        e, s, f = tg._setup(blob, n, iters, precision=PREC_F16X2)
        ie = HnetEngine(ov, variant="prior1", mc_samples=8, dropout_p=0.1, mc_seed=9, max_batch=8, precision=prec)
        _track(e, ie, s, f)
        s.set_iterative_model(ie)
        f.enable_photometric()
        for i in ids:
            f.set_photo_gate(int(i), 0.0 if gates is None else gates[i])
        ti._load(f, s, ps, sts)
        out, net, upd = f.step(ids, [T_FRAME] * n, imus)
        rec = f.last_photometric(n)
        if gates is None:
            ratio = _ratios(rec)
            gates = [0.5 * (ratio[i].min() + ratio[i].max()) for i in range(n)]
            want_at = [_first_over(ratio[i], gates[i]) for i in range(n)]
            assert any(w is not None for w in want_at), ratio
        else:
            assert ie.precision() == PREC_BF16X3 and e.precision() == PREC_F16X2   # (demoted once, the iterative context only)
            assert [s.seq(int(i)) for i in ids] == [iters] * n and np.all(np.isfinite(net))
            assert [int(u) for u in upd] == [iters if w is None else w for w in want_at]
            for i in range(n):
                assert list(rec["flags"][i, 2:]) == [PH_REJECTED if it == want_at[i] else 0 for it in range(iters)]
            stats = [f.photo_stats(int(i)) for i in ids]
            _check_stats(f, ids, [(rec, upd, None)])
            res.append((out, net, upd, rec, stats))
        for o in (f, s, ie, e):
            o.close()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(res[0][:4], res[1][:4])) and res[0][4] == res[1][4]


def test_mixed_advance(blob):
    """h. an advance in which only sessions 6, 1, 3 (listed in that order among all 8) have a new frame and only 1 has a gate: records for exactly those
    three, in listed order, the operator's; 1 is judged and refused, 6 and 3 are never refused"""
    _capi, _, _, HnetFilters = tg._mods()
    iters = 3
    e, s, f = _fleet(blob, iters, innov=False)
    f.enable_feed(64)
    rng = np.random.default_rng(29)
    t_frame = np.full(8, T_FRAME)
    ps, hist = [], []
    for i in range(8):
        p = tg._params(HnetFilters, rng, i)
        f.set_params(i, p)
        f.set_state(i, tg._state(_capi, rng, t_frame[i]))
        ps.append(p)
        ts = t_frame[i] + p.cam_imu_dt - 0.0007 + 0.002 * np.arange(46)
        r = np.zeros(len(ts), _capi.IMU_DTYPE)
        r["t"], r["wm"], r["am"] = ts, rng.standard_normal((len(ts), 3)) * 0.3, rng.standard_normal((len(ts), 3)) * 0.5 + [0, 0, 9.81]
        hist.append(r)
    sub = [6, 1, 3]
    for i in sub:
        t_frame[i] += 0.002 * max(COUNTS[i], 0.1) + 0.0004
    s.push(np.asarray(sub, np.int32), np.repeat(tg._frames(rng, 1), 3, 0), t=[t_frame[i] for i in sub])
    f.feed_imu(np.asarray(sub, np.int32), [hist[i] for i in sub])
    f.set_photo_gate(1, 1e-6)                                                 # any estimate with a residual is worse than a millionth of the prior's
    listed = np.array([6, 0, 1, 2, 3, 4, 5, 7], np.int32)
    out, net, upd, status = f.advance(listed)
    stepped = [int(i) for i, st in zip(listed, status) if st == _capi.ADV_STEPPED]
    assert stepped == sub and all(st == _capi.ADV_NO_FRAME for i, st in zip(listed, status) if int(i) not in sub)
    rec = f.last_photometric(3)
    rows = [int(np.where(listed == i)[0][0]) for i in sub]
    assert _unflag(rec).tobytes() == _operator(e, s, f, sub, net[:, rows, :]).tobytes()
    assert [list(r) for r in rec["flags"]] == [[0] * 5, [0, 0, PH_REJECTED, 0, 0], [0] * 5]
    assert [int(upd[r]) for r in rows] == [iters, 0, iters] and not upd[[r for r in range(8) if r not in rows]].any()
    L = _capi.lib()
    assert L.hnet_filters_last_photometric(f._f, 8, np.zeros((8, 2 + iters), _capi.PHOTO_RESIDUAL_DTYPE).ctypes.data) == INVALID
    got = {i: f.photo_stats(i) for i in range(8)}
    assert (got[1]["judged"], got[1]["rejected"]) == (1, 1) and all((got[i]["judged"], got[i]["rejected"]) == (iters, 0) for i in (6, 3))
    assert all(got[i]["judged"] == 0 for i in (0, 2, 4, 5, 7))
    for o in (f, s, e):
        o.close()


def test_errors(blob):
    """i. set_photo_gate before enable_photometric, with a bad id, a negative or NaN max_ratio or a min_inside out of range: HNET_ERR_INVALID_ARG, and
    nothing changed - the step that follows is the ungated one"""
    _capi, _, _, HnetFilters = tg._mods()
    ea, sa, fa = _track(*tg._setup(blob, 8, 1))
    eb, sb, fb = _track(*tg._setup(blob, 8, 1))
    L = _capi.lib()
    st = _capi.PhotoStats()
    assert L.hnet_filters_set_photo_gate(fa._f, 0, C.c_double(2.0), 0) == INVALID          # before enabling
    assert L.hnet_filters_photo_stats(fa._f, 0, C.byref(st)) == INVALID and L.hnet_filters_reset_photo_stats(fa._f, 0) == INVALID
    fa.enable_photometric()
    fb.enable_photometric()
    for bad_id in (-1, 8):
        assert L.hnet_filters_set_photo_gate(fa._f, bad_id, C.c_double(2.0), 0) == INVALID
        assert L.hnet_filters_photo_stats(fa._f, bad_id, C.byref(st)) == INVALID and L.hnet_filters_reset_photo_stats(fa._f, bad_id) == INVALID
    for bad in (-1.0, float("nan")):
        assert L.hnet_filters_set_photo_gate(fa._f, 0, C.c_double(bad), 0) == INVALID
    for bad_min in (-1, NPIX + 1):
        assert L.hnet_filters_set_photo_gate(fa._f, 0, C.c_double(1e-6), bad_min) == INVALID
    fa.set_photo_gate(3, 1e-6, min_inside=NPIX)
    fa.set_photo_gate(3, 0.0)                                                 # and off again
    ps, sts, imus = ti._inputs(_capi, HnetFilters, 61, 8, T_FRAME, COUNTS)
    ids = np.arange(8, dtype=np.int32)
    for f, s in ((fa, sa), (fb, sb)):
        ti._load(f, s, ps, sts, seq=7)
    a, b = fa.step(ids, [T_FRAME] * 8, imus), fb.step(ids, [T_FRAME] * 8, imus)
    assert _everything(fa, sa, ids, a, False) == _everything(fb, sb, ids, b, False) and list(a[2]) == [1] * 8
    assert not fa.last_photometric(8)["flags"].any()
    for o in (fa, fb, sa, sb, ea, eb):
        o.close()
