"""hnet_filters on the device at the inputs of tests/filters_edges.py, which the benign states and windows of tests/test_gpu_filters.py never reach:
A. an innovation covariance that is singular to the bit (filter_update_kernel's and filter_innovation_kernel's `break`, updates = -1 - done, the reset
   that still runs, SINGULAR / SKIPPED records, the statistics), through hnet_filters_step and hnet_filters_advance, next to partners that must not notice;
B. innovation covariances whose Gauss-Jordan inverse swaps rows on the device, counted from the S the device saw;
C. propagation at the edges of its domain (zero and tiny rates, 35 rad/s, an interval angle past pi, 1 ns intervals, attitudes with w < 0 and at half
   turns, other gravities, the launch file's cam_imu_dt, 400 intervals, a covariance over 12 orders of magnitude) through step, feed + advance and predict.
The references are tests/cpp/filters_ref.cpp, filters_innov_ref.cpp and filters_predict_ref.cpp fed the step's own network outputs; the gates are those of
tests/test_gpu_filters.py (_close: 1e-10) and, for C, the same 1e-10 on the scale of the correlations.  tests/test_filters_edges_cpu.py qualifies the
inputs without a GPU; what depends on the network's outputs (the partners' S, the swaps under the default k_net_cov, the sign margin after an update)
is qualified here from the returned net72."""
import ctypes as C

import numpy as np
import pytest

import filters_edges as fe
import test_gpu_filters as tg
import test_gpu_filters_innov as tgi
import test_gpu_filters_predict as tp
from test_gpu_filters_innov import iref, ref            # noqa: F401  (fixtures)
from test_gpu_filters_predict import pref               # noqa: F401

pytestmark = pytest.mark.gpu

NONE, USED, REJECTED, SINGULAR, SKIPPED = range(5)
ORDER = [0, 4, 1, 5, 2, 6, 3, 7]                         # launch order: singular sessions 0 - 3 and their partners 4 - 7 in neighbouring workgroups
SEQ0 = 7


def _singular_inputs(_capi, HnetFilters, t_state):
    """sessions 0 - 3: the cases of fe.SINGULAR_CASES with k_net_cov = 0; 4 - 7: the same state and parameters with the default k_net_cov"""
    rng = np.random.default_rng(40)
    sts, ps = [], []
    for i in range(4):
        sts.append(fe.singular_state(tg._state(_capi, rng, t_state), rng, fe.SINGULAR_CASES[i][1]))
    sts += [s.copy() for s in sts]
    for i in range(8):
        p = tg._params(HnetFilters, np.random.default_rng(60 + i % 4), i % 4)
        ps.append(p)
    return sts, ps


def _load(f, s, sts, ps, singular):
    for i in range(8):
        p = ps[i]
        k = p.k_net_cov
        if singular and i < 4:
            p.k_net_cov = 0.0
        f.set_params(i, p)
        p.k_net_cov = k
        f.set_state(i, sts[i])
        s.set_seq(i, SEQ0)


def _same_record(dev, want):
    """an innovation record against the header's, byte for byte apart from a NaN's payload"""
    for fld in ("r", "s_diag", "iteration", "flag"):
        assert dev[fld].tobytes() == want[fld].tobytes(), (fld, dev[fld], want[fld])
    assert (np.isnan(dev["nis"]) and np.isnan(want["nis"])) or dev["nis"].tobytes() == want["nis"].tobytes(), (dev["nis"], want["nis"])


def _check_singular_launch(f, s, ref, iref, sts, ps, imus, t_frame, iters, innov, out, net, upd, steps_so_far):
    """what a launch that holds the four singular sessions must give; out / net / upd in launch order ORDER"""
    ids = np.array(ORDER, np.int32)
    assert f.get_state(ids).tobytes() == out.tobytes()
    assert [s.seq(int(i)) for i in ids] == [SEQ0 + iters] * 8                     # the forwards ran for every session in every iteration
    recs = f.last_innovations(8) if innov else None
    for j, i in enumerate(ORDER):
        p = ps[i]
        k = p.k_net_cov
        p.k_net_cov = 0.0 if i < 4 else k
        try:
            want, u = tg._ref_step(ref, sts[i], p, t_frame, imus[i], iters, net[:, j, :], gate=1)
            hs, hu, hrec = tgi._host(ref, iref, sts[i][0], p, t_frame, imus[i], net[:, j, :], 1, 0.0)
        finally:
            p.k_net_cov = k
        assert hu == u and hs.tobytes() == want.tobytes()
        if i < 4:
            name, s8, col = fe.SINGULAR_CASES[i]
            assert fe.gauss_jordan(fe.s_matrix(sts[i]["cov"][0], net[0, j], 0.0)) == (None, [], col), name
            assert upd[j] == u == -1, (name, upd[j], u)
            assert out[j].tobytes() == fe.expected_after_singular(sts[i], t_frame)[0].tobytes(), name
            assert out[j].tobytes() == want[0].tobytes(), name
            if innov:
                assert list(recs["flag"][:, j]) == [SINGULAR] + [SKIPPED] * (iters - 1), (name, recs["flag"][:, j])
                assert np.isnan(recs["nis"][0, j]) and np.array_equal(recs["s_diag"][0, j], np.diag(s8))
                assert not recs["r"][1:, j].any() and not recs["s_diag"][1:, j].any() and not recs["nis"][1:, j].any()
                for it in range(iters):
                    _same_record(recs[it, j], hrec[it])
                st = f.innovation_stats(i)
                assert (st["singular"], st["used"], st["rejected"]) == (steps_so_far, 0, 0), (name, st)
        else:
            assert all(fe.net_cov_is_pd(net[it, j]) for it in range(iters))
            assert upd[j] == u == iters, (i, upd[j], u)
            tg._close(out[j], want[0])
            if innov:
                assert list(recs["flag"][:, j]) == list(hrec["flag"]) == [USED] * iters
                assert max(tgi._rel(recs[fld][:, j], hrec[fld]) for fld in ("r", "s_diag", "nis")) <= tgi.TOL
                st = f.innovation_stats(i)
                assert (st["singular"], st["used"]) == (0, steps_so_far * iters)


@pytest.mark.parametrize("innov", [False, True], ids=["plain", "innov"])
@pytest.mark.parametrize("iters", [1, 3])
def test_singular_s_step(blob, ref, iref, iters, innov):
    """A. two launches with the singular sessions, then one in which the same sessions run with the default k_net_cov: the partners keep their bits"""
    _capi, _, _, HnetFilters = tg._mods()
    e, s, f = tg._setup(blob, 8, iters)
    if innov:
        f.enable_innovations()
    t_frame = fe.T_FRAME
    sts, ps = _singular_inputs(_capi, HnetFilters, t_frame - 0.0004)
    imus = [tg._imu(None, 0.0, 0)] * 8                                             # no readings: the propagation changes nothing
    ids = np.array(ORDER, np.int32)
    first = None
    for launch in (1, 2):
        _load(f, s, sts, ps, singular=True)
        out, net, upd = f.step(ids, [t_frame] * 8, imus)
        _check_singular_launch(f, s, ref, iref, sts, ps, imus, t_frame, iters, innov, out, net, upd, launch)
        first = first or (out, net, upd)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(first, (out, net, upd)))
    _load(f, s, sts, ps, singular=False)
    out, net, upd = f.step(ids, [t_frame] * 8, imus)
    assert list(upd) == [iters] * 8
    partners = [j for j, i in enumerate(ORDER) if i >= 4]
    for j in partners:                                                             # the `break` and the early returns next door disturbed nothing
        assert out[j].tobytes() == first[0][j].tobytes() and net[:, j].tobytes() == first[1][:, j].tobytes() and upd[j] == first[2][j]
    f.close(); s.close(); e.close()


def test_singular_s_advance(blob, ref, iref):
    """A. the same sessions through the device ring and selection (a window inside one pair of readings: no interval), 3 iterations, records on"""
    _capi, _, _, HnetFilters = tg._mods()
    iters = 3
    e, s, f = tg._setup(blob, 8, iters)
    f.enable_innovations()
    f.enable_feed(64)
    t_frame = fe.T_FRAME
    sts, ps = _singular_inputs(_capi, HnetFilters, t_frame - 0.0006)
    ids = np.array(ORDER, np.int32)
    imus = []
    for i in range(8):
        r = np.zeros(2, _capi.IMU_DTYPE)
        r["t"] = float(sts[i]["t"][0]) + ps[i].cam_imu_dt + np.array([-0.0007, 0.0013])
        r["wm"], r["am"] = [0.1, -0.2, 0.3], [0.2, -0.1, 9.8]
        imus.append(r)
    _load(f, s, sts, ps, singular=True)
    f.feed_imu(ids, [imus[i] for i in ORDER])
    out, net, upd, status = f.advance(ids)
    assert list(status) == [_capi.ADV_STEPPED] * 8
    assert [len(f.last_selection(i)) for i in range(8)] == [1] * 8                # one interpolated reading: nothing to integrate
    _check_singular_launch(f, s, ref, iref, sts, ps, imus, t_frame, iters, True, out, net, upd, 1)
    f.close(); s.close(); e.close()


@pytest.mark.parametrize("innov", [False, True], ids=["plain", "innov"])
def test_pivoting_swaps_rows_on_the_device(blob, ref, iref, innov):
    """B. 8 sessions whose S pivots (4 with k_net_cov = 0, 4 with the default), one iteration, no IMU readings: states, updates and (innov) records
    against the host header at the existing gates.  The swap columns are those of the S the device saw; too few of them fail the test.  plain:
    filter_update_kernel's inverse alone; innov: filter_innovation_kernel inverts the same S in front of it."""
    _capi, _, _, HnetFilters = tg._mods()
    n, iters = 8, 1
    e, s, f = tg._setup(blob, n, iters)
    if innov:
        f.enable_innovations()
    t_frame = fe.T_FRAME
    rng = np.random.default_rng(41)
    sts, ps = [], []
    for i in range(n):
        p = tg._params(HnetFilters, rng, i)
        if i in fe.PIVOT_K0:
            p.k_net_cov = 0.0
        st = fe.pivot_state(tg._state(_capi, rng, t_frame - 0.0004), rng, fe.pivot_s8(fe.PIVOT_PERMS[i]))
        f.set_params(i, p)
        f.set_state(i, st)
        ps.append(p)
        sts.append(st)
    imus = [tg._imu(None, 0.0, 0)] * n
    ids = np.arange(n, dtype=np.int32)
    out, net, upd = f.step(ids, [t_frame] * n, imus)
    recs = f.last_innovations(n) if innov else None
    cols, worst = set(), {"mean": 0.0, "cov": 0.0, "corr": 0.0, "r": 0.0, "s_diag": 0.0, "nis": 0.0}
    for i in range(n):
        want, u, rec = tgi._host(ref, iref, sts[i][0], ps[i], t_frame, imus[i], net[:, i, :], 1, 0.0)
        prop = sts[i].copy()
        assert ref.ref_propagate_with_imu(C.c_void_p(prop.ctypes.data), C.byref(ps[i]), C.c_double(t_frame), None, 0) == 0
        S = fe.s_matrix(prop["cov"][0], net[0, i], ps[i].k_net_cov)
        inv, swaps, col = fe.gauss_jordan(S)
        print(f"pivot session {i}: k_net_cov {ps[i].k_net_cov:g}, cond {np.linalg.cond(S):.3g}, swaps in columns {swaps}; state dev mean "
              f"{fe.mean_dev(out[i], want[0]):.3e} cov {fe.cov_dev_max(out[i]['cov'], want[0]['cov']):.3e} corr {fe.cov_dev_corr(out[i]['cov'], want[0]['cov']):.3e}")
        assert col is None and len(swaps) >= fe.MIN_SWAPS, (i, swaps)
        cols |= set(swaps)
        assert upd[i] == u == 1 and list(rec["flag"]) == [USED]
        assert not innov or list(recs["flag"][:, i]) == [USED]
        worst["mean"] = max(worst["mean"], fe.mean_dev(out[i], want[0]))
        worst["cov"] = max(worst["cov"], fe.cov_dev_max(out[i]["cov"], want[0]["cov"]))
        worst["corr"] = max(worst["corr"], fe.cov_dev_corr(out[i]["cov"], want[0]["cov"]))
        for fld in ("r", "s_diag", "nis") if innov else ():
            worst[fld] = max(worst[fld], tgi._rel(recs[fld][:, i], rec[fld]))
    print(f"pivoting: {len(cols)} distinct swap columns {sorted(cols)}; largest differences {worst}")
    assert len(cols) >= fe.MIN_SWAP_COLUMNS, cols
    for i in range(n):
        want, _u, _rec = tgi._host(ref, iref, sts[i][0], ps[i], t_frame, imus[i], net[:, i, :], 1, 0.0)
        tg._close(out[i], want[0])
    assert max(worst["r"], worst["s_diag"], worst["nis"]) <= tgi.TOL, worst
    f.close(); s.close(); e.close()


# ---------------------------------------------------------------------------------------------- C
def _edge_chunks():
    ses = fe.edge_sessions()
    return [ses[:9], ses[9:]]


def _judge(label, rows):
    """rows: (case id, device state, host state).  Prints every case's largest deviation on both scales, then applies _close and the correlation gate."""
    for cid, dev, want in rows:
        print(f"{label} {cid:18s} mean {fe.mean_dev(dev, want):.3e}  cov/max|P| {fe.cov_dev_max(dev['cov'], want['cov']):.3e}  "
              f"cov/corr {fe.cov_dev_corr(dev['cov'], want['cov']):.3e}")
    for cid, dev, want in rows:
        tg._close(dev, want)
        assert fe.cov_dev_corr(dev["cov"], want["cov"]) <= tg.TOL_COV, (cid, fe.cov_dev_corr(dev["cov"], want["cov"]))


def _host_edge(ref, ses, net_i):
    """the host reference of one session's step and the sign margin along it: q's last component after every interval and after the update"""
    want, u = tg._ref_step(ref, ses["st"], ses["p"], fe.T_FRAME, ses["imu"], 1, net_i, gate=1)
    _st, q, _ang = fe.trace(ref, ses)
    margin = min(float(np.abs(q[:, 3]).min()), float(abs(want["q"][0][3])))
    assert margin >= fe.R3_MARGIN, (ses["id"], margin)                             # a case that comes this near the flip is to be replaced, not tolerated
    return want, u


def test_edges_step_matches_host_reference(blob, ref):
    """C. the 17 sessions of fe.EDGE_CASES in two steps (9 and 8 sessions), one iteration, the reference gate open"""
    rows = []
    for chunk in _edge_chunks():
        n = len(chunk)
        e, s, f = tg._setup(blob, n, 1, max_batch=16)
        for i, ses in enumerate(chunk):
            f.set_params(i, ses["p"])
            f.set_state(i, ses["st"])
        ids = np.arange(n, dtype=np.int32)
        out, net, upd = f.step(ids, [fe.T_FRAME] * n, [ses["imu"] for ses in chunk])
        assert f.get_state(ids).tobytes() == out.tobytes()
        for i, ses in enumerate(chunk):
            want, u = _host_edge(ref, ses, net[:, i, :])
            assert upd[i] == u == 1, (ses["id"], upd[i], u)
            assert np.all(np.isfinite(out[i]["cov"])) and np.all(out[i]["offset"] == 0) and np.all(out[i]["cov"][15:, :] == 0)
            rows.append((ses["id"], out[i], want[0]))
        f.close(); s.close(); e.close()
    _judge("step", rows)


def test_edges_advance_matches_host_reference(blob, ref):
    """C. the same readings through feed_imu and advance on rings of 512 readings that wrap: full after the older readings, the window written over
    the oldest of them"""
    _capi = tg._mods()[0]
    rows, same = [], []
    for chunk in _edge_chunks():
        n = len(chunk)
        e, s, f = tg._setup(blob, n, 1, max_batch=16)
        f.enable_feed(fe.RING)
        for i, ses in enumerate(chunk):
            f.set_params(i, ses["p"])
            f.set_state(i, ses["st"])
        ids = np.arange(n, dtype=np.int32)
        f.feed_imu(ids, [ses["imu"][:fe.PREFIX] for ses in chunk])
        f.feed_imu(ids, [ses["imu"][fe.PREFIX:] for ses in chunk])
        out, net, upd, status = f.advance(ids)
        assert list(status) == [_capi.ADV_STEPPED] * n
        for i, ses in enumerate(chunk):
            assert len(f.last_selection(i)) == ses["n_int"] + 1, ses["id"]
            want, u = _host_edge(ref, ses, net[:, i, :])
            assert upd[i] == u == 1, (ses["id"], upd[i], u)
            rows.append((ses["id"], out[i], want[0]))
        f.close(); s.close(); e.close()
    _judge("advance", rows)


def test_edges_predict_matches_host_header(blob, pref):
    """C. the zero-rate and the 35 rad/s sessions predicted to their frame's time from the rings, against filters_predict_ref"""
    _capi = tg._mods()[0]
    chunk = _edge_chunks()[0]
    n = len(chunk)
    e, s, f = tg._setup(blob, n, 1, max_batch=16)
    f.enable_feed(fe.RING)
    for i, ses in enumerate(chunk):
        f.set_params(i, ses["p"])
        f.set_state(i, ses["st"])
    ids = np.arange(n, dtype=np.int32)
    f.feed_imu(ids, [ses["imu"][:fe.PREFIX] for ses in chunk])
    f.feed_imu(ids, [ses["imu"][fe.PREFIX:] for ses in chunk])
    sel = np.array([i for i, ses in enumerate(chunk) if ses["id"] in fe.PREDICT_IDS], np.int32)
    assert len(sel) == len(fe.PREDICT_IDS)
    o = f.predict(sel, [fe.T_FRAME] * len(sel))
    worst = 0.0
    for k, i in enumerate(sel):
        ses = chunk[i]
        want = np.zeros(1, _capi.ODOMETRY_DTYPE)
        r = np.ascontiguousarray(ses["imu"])
        pref.pred_ref_predict(ses["st"].ctypes.data, C.addressof(ses["p"]), float(fe.T_FRAME), r.ctypes.data, len(r), want.ctypes.data)
        assert o[k]["status"] == want[0]["status"] == _capi.PRED_OK and o[k]["intervals"] == want[0]["intervals"] == ses["n_int"], ses["id"]
        d = tp._rel(o[k], want[0])
        print(f"predict {ses['id']:18s} largest relative difference {d:.3e}")
        worst = max(worst, d)
    assert worst <= tp.TOL, worst
    f.close(); s.close(); e.close()
