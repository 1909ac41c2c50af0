"""hnet_filters_predict_cov (include/hnet.h): hnet_filters_predict's record plus the covariance propagated to the same query time, read-only.
The covariance must be, bit for bit, what the advance that follows computes before its reset (rows and columns 0 .. 14 of its state_out; the offset
block through iteration 0's innovation record with k_net_cov = 0); the record must be hnet_filters_predict's, byte for byte; everything must agree with
the host header (tests/cpp/filters_predict_cov_ref.cpp) on the same history at the gates of tests/test_gpu_filters.py; nothing may be written; the
statuses and errors are the predict's.  Setup: the Fleet of tests/test_gpu_filters_predict.py (8 sessions, max_batch 8, rings of 64 that have wrapped,
windows of COUNTS intervals: none, one, a wrapped span, the longest window), random dense 27 x 27 initial covariances."""
import ctypes as C

import numpy as np
import pytest

import filters_edges as fe
import test_filters_predict_cov_cpu as cc
import test_gpu_filters as tg
import test_gpu_filters_innov as tgi
import test_gpu_filters_predict as tp
from test_filters_predict_cov_cpu import cref           # noqa: F401  (fixtures)
from test_gpu_filters_innov import iref, ref            # noqa: F401

pytestmark = pytest.mark.gpu

T0 = tp.T0
BLOCKS = ("pose_cov", "body_pos_cov", "body_vel_cov", "prior_cov_px")
SEL = fe.SEL


def _host(fl, cref, states, t_query, hist=None):
    """pcov_ref_predict per session on everything it was fed (or on hist[i])"""
    A = fl.capi
    out, cov, full = np.zeros(8, A.ODOMETRY_DTYPE), np.zeros(8, A.ODOMETRY_COV_DTYPE), np.zeros((8, 27, 27))
    for i in range(8):
        r = np.ascontiguousarray(fl.hist[i][:fl.fed[i]] if hist is None else hist[i])
        cref.pcov_ref_predict(states[i:i + 1].ctypes.data, C.addressof(fl.ps[i]), float(t_query[i]), r.ctypes.data, len(r), out[i:].ctypes.data,
                              cov[i:].ctypes.data, full[i:].ctypes.data)
    return out, cov, full


def _host_blocks(fl, cref, state):
    oc = np.zeros(1, fl.capi.ODOMETRY_COV_DTYPE)
    cref.pcov_ref_odometry_cov(state.ctypes.data, oc.ctypes.data)
    return oc


def _compare(dev, want, live):
    """(mean fields, full on the scale of max |P|, full on the correlation scale, the derived blocks on their own largest element): the largest
    difference of each kind over the sessions `live`"""
    (o, oc, full), (ho, hoc, hfull) = dev, want
    m = max(tp._rel(o[i], ho[i]) for i in live)
    c = max(fe.cov_dev_max(full[i], hfull[i]) for i in live)
    r = max(fe.cov_dev_corr(full[i], hfull[i]) for i in live)
    b = max(float(np.abs(oc[i][k] - hoc[i][k]).max() / np.abs(hoc[i][k]).max()) for i in live for k in BLOCKS)
    return m, c, r, b


def test_predict_cov_equals_the_advance_that_follows(blob):
    """filter_propagate_kernel's operations in its order under -ffp-contract=off: equality is bitwise"""
    fl = tp.Fleet(blob)
    A = fl.capi
    t_f = fl.next_frame()
    init = fl.f.get_state(fl.ids)
    plain = fl.f.predict(fl.ids, t_f)
    o, oc, full = fl.f.predict_cov(fl.ids, t_f, full=True)
    sta, net, upd, status = fl.f.advance(fl.ids)
    assert list(status) == [A.ADV_STEPPED] * 8 and list(upd) == [0] * 8             # gate closed: propagated, forward, no update, reset
    assert list(o["status"]) == [A.PRED_OK] * 8
    assert o.tobytes() == plain.tobytes()
    pri = fl.f.last_priors(8)[0]
    for i in range(8):
        for fld in ("p", "q", "v"):
            assert o[i][fld].tobytes() == sta[i][fld].tobytes(), (i, fld)
        assert np.ascontiguousarray(full[i][:15, :15]).tobytes() == np.ascontiguousarray(sta[i]["cov"][:15, :15]).tobytes(), i
        assert not sta[i]["cov"][15:, :].any() and not sta[i]["cov"][:, 15:].any()    # the closing reset touched rows and columns from 15 on, only
        assert o[i]["prior_px"].astype(np.float32).tobytes() == pri[i].tobytes(), i
        assert o[i]["intervals"] == len(fl.f.last_selection(i)) - 1, i
    assert o["intervals"][0] == 0 and o["intervals"][1] == 2 and o["intervals"][4] == 41       # no interval, a short window, the longest
    moved = np.abs(full[4][:15, :15] - init[4]["cov"][:15, :15]).max() / np.abs(init[4]["cov"]).max()
    print(f"40-interval session: the IMU block moved by {moved:.3e} of the largest initial element")
    assert moved > 1e-3
    assert full[0].tobytes() == init[0]["cov"].tobytes()                              # no interval: the state's covariance bytes
    assert np.abs(full[:, 15:, 15:]).max() > 0                                         # the offset block is there: before any reset
    fl.close()


def test_offset_block_equals_the_s_the_update_forms(blob, ref, iref):
    """2 sessions with 12 images (the reference gate is open), k_net_cov = 0: iteration 0's S is P[sel, sel] at the frame's time itself"""
    _capi, _, _, HnetFilters = tg._mods()
    e, s, f = tg._setup(blob, 2, 1, max_batch=2)
    f.enable_innovations()
    f.enable_feed(64)
    t_frame = fe.T_FRAME
    ps, sts, imus = tgi._inputs(_capi, HnetFilters, 5, 2, t_frame, [16, 3])
    for p in ps:
        p.k_net_cov = 0.0
    tgi._load(f, s, ps, sts)
    ids = np.arange(2, dtype=np.int32)
    f.feed_imu(ids, imus)
    o, oc, full = f.predict_cov(ids, [t_frame] * 2, full=True)
    out, net, upd, status = f.advance(ids)
    assert list(status) == [_capi.ADV_STEPPED] * 2 and list(upd) == [1, 1] and list(o["status"]) == [_capi.PRED_OK] * 2
    assert list(o["intervals"]) == [len(f.last_selection(i)) - 1 for i in range(2)] and min(o["intervals"]) > 2
    recs = f.last_innovations(2)
    for i in range(2):
        hs, hu, hrec = tgi._host(ref, iref, sts[i][0], ps[i], t_frame, imus[i], net[:, i, :], 1, 0.0)
        assert hu == 1 and hrec["flag"][0] == tgi.USED                                # a singular draw would be a bad input, not a pass
        assert recs["flag"][0, i] == tgi.USED
        d = np.ascontiguousarray(np.diag(full[i][np.ix_(SEL, SEL)]))
        assert recs["s_diag"][0, i].tobytes() == d.tobytes(), (i, recs["s_diag"][0, i], d)
        assert np.ascontiguousarray(np.diag(oc[i]["prior_cov_px"])).tobytes() == (159.5 * 159.5 * d).tobytes()
        assert d.min() > 0
    f.close(); s.close(); e.close()


def test_predict_cov_matches_host_header(blob, cref):
    fl = tp.Fleet(blob)
    t_f = fl.next_frame()
    states = fl.f.get_state(fl.ids)
    dev = fl.f.predict_cov(fl.ids, t_f, full=True)
    want = _host(fl, cref, states, t_f)
    assert list(dev[0]["status"]) == list(want[0]["status"]) == [fl.capi.PRED_OK] * 8
    assert list(dev[0]["intervals"]) == list(want[0]["intervals"])
    m, c, r, b = _compare(dev, want, range(8))
    equal = all(x.tobytes() == y.tobytes() for x, y in zip(dev, want))
    print(f"predict_cov, device vs host header: mean {m:.3e}, full covariance {c:.3e} of max |P|, {r:.3e} on the correlation scale, derived blocks {b:.3e}"
          f" (bounds {tg.TOL_MEAN:.0e} / {tg.TOL_COV:.0e}); bitwise equal: {equal}")
    assert m <= tg.TOL_MEAN and c <= tg.TOL_COV and r <= tg.TOL_COV and b <= tg.TOL_COV, (m, c, r, b)
    fl.close()


def test_predict_cov_is_read_only(blob):
    """two fleets run the same 5 ticks; one of them calls predict_cov (full) and predict between the feed and the advance of every tick"""
    a, b = tp.Fleet(blob), tp.Fleet(blob)
    for tick in range(5):
        t_f = a.next_frame()
        b.next_frame()
        before = a.snapshot() if tick else None                                      # (last_priors needs a first advance)
        o, oc, full = a.f.predict_cov(a.ids, t_f, full=True)
        plain = a.f.predict(a.ids, t_f)
        o2, oc2 = a.f.predict_cov(a.ids, t_f)
        assert list(o["status"]) == [a.capi.PRED_OK] * 8
        assert o.tobytes() == plain.tobytes() == o2.tobytes() and oc.tobytes() == oc2.tobytes()
        if tick:
            assert a.snapshot() == before
        ra, rb = a.f.advance(a.ids), b.f.advance(b.ids)
        for x, y in zip(ra, rb):                                                     # states, net_out, updates, statuses
            assert x.tobytes() == y.tobytes(), tick
        sa, sb = a.snapshot(), b.snapshot()
        assert sa[:5] == sb[:5] and sa[5]["n_steps"] == sb[5]["n_steps"] == tick + 1 and sa[5]["n_inferences"] == sb[5]["n_inferences"]
    a.close(); b.close()


def test_statuses_and_errors(blob, cref):
    fl = tp.Fleet(blob, inited=range(7))                                             # session 7 has no state
    A, f = fl.capi, fl.f
    o, oc, full = f.predict_cov([0], [T0 + 0.01], full=True)                         # nothing fed yet
    assert list(o["status"]) == [A.PRED_WAIT_IMU] and not full.any() and not oc.tobytes().strip(b"\0")
    t_f = fl.next_frame()
    states = f.get_state(fl.ids)
    newest = np.array([f.newest_imu_time(i) for i in range(8)])
    dt = np.array([p.cam_imu_dt for p in fl.ps])
    tq = t_f.copy()
    tq[2] = newest[2] - dt[2]                                                        # at the newest reading
    tq[3] = newest[3] - dt[3] + 0.5                                                  # beyond it
    tq[4] = T0                                                                       # at the state
    tq[5] = T0 - 1.0                                                                 # before it
    o, oc, full = f.predict_cov(fl.ids, tq, full=True)                               # mixed statuses in one call
    assert list(o["status"]) == [A.PRED_OK, A.PRED_OK, A.PRED_WAIT_IMU, A.PRED_WAIT_IMU, A.PRED_AT_STATE, A.PRED_AT_STATE, A.PRED_OK, A.PRED_NO_STATE]
    assert o.tobytes() == f.predict(fl.ids, tq).tobytes()
    zero = np.zeros(1, A.ODOMETRY_DTYPE)
    for i in (2, 3, 7):
        zero["status"] = o[i]["status"]
        assert o[i].tobytes() == zero[0].tobytes() and not oc[i].tobytes().strip(b"\0") and not full[i].any()
    for i in (4, 5):
        assert full[i].tobytes() == states[i]["cov"].tobytes()
        assert oc[i].tobytes() == _host_blocks(fl, cref, states[i:i + 1])[0].tobytes()
        assert o[i]["t_cam"] == T0 and o[i]["intervals"] == 0
    ok = [0, 1, 6]
    for i in ok:
        assert full[i].tobytes() != states[i]["cov"].tobytes() or o[i]["intervals"] == 0
    for i in ok:                                                                     # n = 1, with and without the full covariance
        a1 = f.predict_cov([i], tq[i:i + 1], full=True)
        b1 = f.predict_cov([i], tq[i:i + 1])
        assert a1[0].tobytes() == b1[0].tobytes() == o[i:i + 1].tobytes() and a1[1].tobytes() == b1[1].tobytes() == oc[i:i + 1].tobytes()
        assert a1[2].tobytes() == full[i:i + 1].tobytes()
    # errors: the code, and nothing written
    L = A.lib()
    f2 = type(f)(fl.s, 1)                                                            # a filters object without enable_feed
    bad = [(f._f, [0, 0], 1), (f._f, [8], 1), (f._f, [-1], 1), (f._f, list(range(8)) + [0], 5), (f2._f, [0], 1), (f._f, [], 1)]
    snap = f.get_state(fl.ids).tobytes()

    def call(handle, ids, tq1, null=None):
        n = max(len(ids), 1)
        bufs = [np.full(n * A.ODOMETRY_DTYPE.itemsize, 0xA5, np.uint8), np.full(n * A.ODOMETRY_COV_DTYPE.itemsize, 0xA5, np.uint8),
                np.full(n * 729 * 8, 0xA5, np.uint8)]
        ptr = [None if k == null else x.ctypes.data for k, x in enumerate(bufs)]
        code = L.hnet_filters_predict_cov(handle, len(ids), ids.ctypes.data, tq1.ctypes.data, *ptr)
        assert all(np.all(x == 0xA5) for x in bufs)
        return code

    for handle, ids, code in bad:
        ids = np.array(ids, np.int32)
        assert call(handle, ids, np.full(max(len(ids), 1), T0 + 0.001)) == code, ids
    one = np.zeros(1, np.int32)
    assert call(f._f, one, np.array([np.nan])) == 1 and call(f._f, one, np.array([np.inf])) == 1
    assert call(f._f, one, np.array([T0 + 0.001]), null=0) == 1 and call(f._f, one, np.array([T0 + 0.001]), null=1) == 1
    assert f.get_state(fl.ids).tobytes() == snap
    with pytest.raises(A.HnetError):
        f.predict_cov([0, 0], [T0 + 0.001] * 2)
    f2.close()
    fl.close()


def test_window_further_back_than_the_ring(blob, cref):
    """three frames without an advance: the 40-interval session's window (120 intervals) starts before the oldest of the ring's 64 readings; the
    device propagates with what is there, as the header does when it is fed what the ring still holds"""
    fl = tp.Fleet(blob)
    for _ in range(3):
        t_f = fl.next_frame()
    states = fl.f.get_state(fl.ids)
    assert float(states[4]["t"]) == T0
    held = [fl.hist[i][max(fl.fed[i] - 64, 0):fl.fed[i]] for i in range(8)]
    assert held[4]["t"][0] > T0 + fl.ps[4].cam_imu_dt + 0.05                          # the window's start is no longer in the ring
    dev = fl.f.predict_cov(fl.ids, t_f, full=True)
    want = _host(fl, cref, states, t_f, hist=held)
    assert list(dev[0]["status"]) == list(want[0]["status"]) == [fl.capi.PRED_OK] * 8
    assert list(dev[0]["intervals"]) == list(want[0]["intervals"]) and dev[0]["intervals"][4] >= 60
    m, c, r, b = _compare(dev, want, range(8))
    print(f"window past the ring, device vs host header on the ring's readings: mean {m:.3e}, covariance {c:.3e} / {r:.3e}, blocks {b:.3e}")
    assert m <= tg.TOL_MEAN and c <= tg.TOL_COV and r <= tg.TOL_COV and b <= tg.TOL_COV, (m, c, r, b)
    fl.close()
