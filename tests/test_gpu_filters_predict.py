"""hnet_filters_predict (include/hnet.h): the states of the listed sessions predicted to a query time from the device's IMU rings, read-only.  A
predict to a pending frame's time must give, bit for bit, the mean and the prior the advance that follows computes; it must agree with the host
header (tests/cpp/filters_predict_ref.cpp) on the same history; it must leave every piece of state and bookkeeping as it was; its statuses and
errors.  Setup throughout: prior-3, N = 16, max_batch 8, 8 sessions with 2 - 9 images, rings of 64 readings that have wrapped, windows of
0 - 40 intervals per session, cam_imu_dt / imu_avg varied (the setup of tests/test_gpu_filters_feed.py::test_feed_equals_step)."""
import ctypes as C

import numpy as np
import pytest

import test_filters_cpu as tc
import test_filters_predict_cpu as pc
import test_gpu_filters as tg

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 2, 16, 40, 16, 3, 7]
T0 = 3.0
ODO_FIELDS = ("t_cam", "t_imu", "p", "q", "v", "w_pos", "rpy", "body_pos", "body_vel", "prior_px")
TOL = tg.TOL_MEAN                      # 1e-10, relative in the sense of test_gpu_filters._close: the device and the host differ in sin / cos / sqrt / division only


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return pc.build_ref(str(tmp_path_factory.mktemp("filters_predict_ref") / "filters_predict_ref.so"))


class Fleet:
    """8 sessions (session i holds 2 + i images: the gate stays closed), states at T0, per session one IMU stream that starts 70 readings before T0
    (so every ring of 64 has wrapped once the first window is handed over) and runs on for the ticks of a test"""

    def __init__(self, blob, inited=range(8)):
        _capi, HnetEngine, HnetSessions, HnetFilters = tg._mods()
        self.capi = _capi
        self.e, self.s, self.f = tg._setup(blob, 8, 1, frames=2)
        self.f.enable_feed(64)
        rng = np.random.default_rng(31)
        self.rng = rng
        self.ids = np.arange(8, dtype=np.int32)
        fr = tg._frames(rng, 7)
        for k in range(7):
            sub = self.ids[k + 1:]
            self.s.push(sub, np.repeat(fr[k][None], len(sub), 0), t=[1.3 + 0.1 * k] * len(sub))
        self.ps, self.hist, self.fed = [], [], [0] * 8
        for i in range(8):
            p = tg._params(HnetFilters, rng, i)
            self.f.set_params(i, p)
            if i in inited:
                self.f.set_state(i, tg._state(_capi, rng, T0))
            self.ps.append(p)
            ts = T0 + p.cam_imu_dt - 0.0007 + 0.002 * np.arange(-70, 5 * 42 + 4)
            r = np.zeros(len(ts), _capi.IMU_DTYPE)
            r["t"], r["wm"], r["am"] = ts, rng.standard_normal((len(ts), 3)) * 0.3, rng.standard_normal((len(ts), 3)) * 0.5 + [0, 0, 9.81]
            self.hist.append(r)
        self.t_frame = np.full(8, T0)
        self.frames = tg._frames(rng, 6)
        self.tick = 0

    def next_frame(self):
        """the next frame of every session (0 - 40 intervals past the last) and the readings that have arrived by then: up to the first one past it"""
        self.t_frame = self.t_frame + 0.002 * np.maximum(COUNTS, 0.1) + 0.0004
        self.s.push(self.ids, np.repeat(self.frames[self.tick][None], 8, 0), t=list(self.t_frame))
        self.tick += 1
        chunks = []
        for i in range(8):
            upto = int(np.searchsorted(self.hist[i]["t"], self.t_frame[i] + self.ps[i].cam_imu_dt, side="right")) + 1
            chunks.append(self.hist[i][self.fed[i]:upto])
            self.fed[i] = upto
        self.f.feed_imu(self.ids, chunks)
        return self.t_frame.copy()

    def host(self, pref, states, t_query):
        """pred_ref_predict per session on everything it was fed"""
        out = np.zeros(8, self.capi.ODOMETRY_DTYPE)
        for i in range(8):
            r = np.ascontiguousarray(self.hist[i][:self.fed[i]])
            pref.pred_ref_predict(states[i:i + 1].ctypes.data, C.addressof(self.ps[i]), float(t_query[i]), r.ctypes.data, len(r), out[i:].ctypes.data)
        return out

    def snapshot(self):
        f, s = self.f, self.s
        return (f.get_state(self.ids).tobytes(), [f.last_selection(i).tobytes() for i in range(8)], f.last_priors(8).tobytes(),
                [s.seq(i) for i in range(8)], [s.image_count(i) for i in range(8)], f.last_timing(), s.last_timing(),
                [f.newest_imu_time(i) for i in range(8)], [f.initialized(i) for i in range(8)])

    def close(self):
        for o in (self.f, self.s, self.e):
            o.close()


def _rel(dev, want):
    worst = 0.0
    for fld in ODO_FIELDS:
        d, w = np.asarray(dev[fld], float), np.asarray(want[fld], float)
        worst = max(worst, float(np.abs(d - w).max() / max(1.0, np.abs(w).max())))
    return worst


def test_predict_equals_the_advance_that_follows(blob):
    """the same device functions in the same order under -ffp-contract=off: equality is bitwise"""
    fl = Fleet(blob)
    A = fl.capi
    t_f = fl.next_frame()
    o = fl.f.predict(fl.ids, t_f)
    sta, net, upd, status = fl.f.advance(fl.ids)
    assert list(status) == [A.ADV_STEPPED] * 8 and list(upd) == [0] * 8             # gate closed: propagated, forward, no update
    assert list(o["status"]) == [A.PRED_OK] * 8
    pri = fl.f.last_priors(8)[0]
    for i in range(8):
        for fld in ("p", "q", "v"):
            assert o[i][fld].tobytes() == sta[i][fld].tobytes(), (i, fld, o[i][fld], sta[i][fld])
        assert o[i]["prior_px"].astype(np.float32).tobytes() == pri[i].tobytes(), (i, o[i]["prior_px"], pri[i])
        assert o[i]["intervals"] == len(fl.f.last_selection(i)) - 1, i
        assert o[i]["t_cam"] == t_f[i] == sta[i]["t"] and o[i]["t_imu"] == t_f[i] + fl.ps[i].cam_imu_dt
    # what the reference's selection gives on what was fed (numpy restatement of Propagator.cpp:81-175): session 0's window lies inside one pair of
    # readings and only one reading past the frame has arrived, so it closes with a single reading and no interval, in the advance as here
    want = []
    for i in range(8):
        rows = fl.hist[i][:fl.fed[i]].view(np.float64).reshape(-1, 7)
        want.append(max(len(tc.np_select(list(rows), T0 + fl.ps[i].cam_imu_dt, t_f[i] + fl.ps[i].cam_imu_dt)) - 1, 0))
    assert list(o["intervals"]) == want and min(want) == 0 and max(want) == 41, (list(o["intervals"]), want)
    assert np.abs(o["prior_px"]).max() > 0.1
    fl.close()


def test_predict_matches_host_header(blob, pref):
    fl = Fleet(blob)
    t_f = fl.next_frame()
    states = fl.f.get_state(fl.ids)
    o = fl.f.predict(fl.ids, t_f)
    want = fl.host(pref, states, t_f)
    assert list(o["status"]) == list(want["status"]) == [fl.capi.PRED_OK] * 8
    assert list(o["intervals"]) == list(want["intervals"])
    worst = max(_rel(o[i], want[i]) for i in range(8))
    print(f"predict, device vs host header: largest relative difference {worst:.3e} (bound {TOL:.0e})")
    assert worst <= TOL, worst
    fl.close()


def test_predict_is_read_only(blob):
    """two fleets run the same 5 ticks; one of them predicts between the feed and the advance of every tick (and again after the advance)"""
    a, b = Fleet(blob), Fleet(blob)
    for tick in range(5):
        t_f = a.next_frame()
        b.next_frame()
        if tick:                                                                     # (last_priors needs a first advance)
            before = a.snapshot()
            o = a.f.predict(a.ids, t_f)
            assert list(o["status"]) == [a.capi.PRED_OK] * 8
            assert a.snapshot() == before
        else:
            a.f.predict(a.ids, t_f)
        ra, rb = a.f.advance(a.ids), b.f.advance(b.ids)
        for x, y in zip(ra, rb):
            assert x.tobytes() == y.tobytes(), tick
        after = a.snapshot()
        o = a.f.predict(a.ids, t_f - 1e-4)                                           # behind the new state: the state as it is
        assert list(o["status"]) == [a.capi.PRED_AT_STATE] * 8
        assert a.snapshot() == after
        sa, sb = after, b.snapshot()
        assert sa[:5] == sb[:5] and sa[5]["n_steps"] == sb[5]["n_steps"] == tick + 1 and sa[5]["n_inferences"] == sb[5]["n_inferences"]
    a.close(); b.close()


def test_statuses_and_errors(blob):
    fl = Fleet(blob, inited=range(7))                                                # session 7 has no state
    A, f = fl.capi, fl.f
    assert np.isnan(f.newest_imu_time(0)) and np.isnan(f.newest_imu_time(99))
    o = f.predict([0], [T0 + 0.01])                                                  # nothing fed yet
    assert list(o["status"]) == [A.PRED_WAIT_IMU]
    t_f = fl.next_frame()
    states = f.get_state(fl.ids)
    newest = np.array([f.newest_imu_time(i) for i in range(8)])
    assert [newest[i] == fl.hist[i]["t"][fl.fed[i] - 1] for i in range(8)] == [True] * 8
    dt = np.array([p.cam_imu_dt for p in fl.ps])
    tq = t_f.copy()
    tq[2] = newest[2] - dt[2]                                                        # at the newest reading
    tq[3] = newest[3] - dt[3] + 0.5                                                  # beyond it
    tq[4] = T0                                                                       # at the state
    tq[5] = T0 - 1.0                                                                 # before it
    o = f.predict(fl.ids, tq)
    assert list(o["status"]) == [A.PRED_OK, A.PRED_OK, A.PRED_WAIT_IMU, A.PRED_WAIT_IMU, A.PRED_AT_STATE, A.PRED_AT_STATE, A.PRED_OK, A.PRED_NO_STATE]
    zero = np.zeros(1, A.ODOMETRY_DTYPE)
    for i in (2, 3, 7):
        zero["status"] = o[i]["status"]
        assert o[i].tobytes() == zero[0].tobytes()
    for i in (4, 5):
        for fld in ("p", "q", "v"):
            assert o[i][fld].tobytes() == states[i][fld].tobytes()
        assert o[i]["t_cam"] == T0 and o[i]["t_imu"] == T0 + dt[i] and o[i]["intervals"] == 0
        assert o[i]["prior_px"].tobytes() == (states[i]["offset"][:, :2].reshape(8) * 159.5).tobytes()
    ok = [0, 1, 6]
    alone = f.predict(ok, tq[ok])
    assert alone.tobytes() == o[ok].tobytes() and np.all(alone["intervals"][1:] > 0) and np.abs(alone["p"] - states[ok]["p"]).max() > 0
    # errors: the code, and nothing written
    L = A.lib()
    f2 = type(f)(fl.s, 1)                                                            # a filters object without enable_feed
    bad = [(f._f, [0, 0], 1), (f._f, [8], 1), (f._f, [-1], 1), (f._f, list(range(8)) + [0], 5), (f2._f, [0], 1), (f._f, [], 1)]
    snap = f.get_state(fl.ids).tobytes()
    for handle, ids, code in bad:
        ids = np.array(ids, np.int32)
        out = np.full(max(len(ids), 1) * A.ODOMETRY_DTYPE.itemsize, 0xA5, np.uint8)
        tq1 = np.full(max(len(ids), 1), T0 + 0.001)
        assert L.hnet_filters_predict(handle, len(ids), ids.ctypes.data, tq1.ctypes.data, out.ctypes.data) == code, ids
        assert np.all(out == 0xA5)
    out = np.full(A.ODOMETRY_DTYPE.itemsize, 0xA5, np.uint8)
    one = np.zeros(1, np.int32)
    assert L.hnet_filters_predict(f._f, 1, one.ctypes.data, np.array([np.nan]).ctypes.data, out.ctypes.data) == 1 and np.all(out == 0xA5)
    assert f.get_state(fl.ids).tobytes() == snap
    with pytest.raises(A.HnetError):
        f.predict([0, 0], [T0 + 0.001] * 2)
    f2.close()
    fl.close()


def test_three_predicts_in_one_gap(blob, pref):
    """increasing query times inside one inter-frame gap, each from the unchanged state: the call's scratch is reused, the spans wrap"""
    fl = Fleet(blob)
    t_f = fl.next_frame()
    fl.f.advance(fl.ids)
    t_prev, t_f = t_f, fl.next_frame()                                              # second tick: the windows lie across the rings' wrap points
    states = fl.f.get_state(fl.ids)
    worst, seen = 0.0, []
    for frac in (0.3, 0.7, 1.0):
        tq = t_prev + frac * (t_f - t_prev)
        o = fl.f.predict(fl.ids, tq)
        want = fl.host(pref, states, tq)
        assert list(o["status"]) == [fl.capi.PRED_OK] * 8 and list(o["intervals"]) == list(want["intervals"])
        worst = max(worst, max(_rel(o[i], want[i]) for i in range(8)))
        seen.append(o["intervals"].copy())
        assert fl.f.get_state(fl.ids).tobytes() == states.tobytes()
    assert np.all(seen[0] <= seen[1]) and np.all(seen[1] <= seen[2]) and seen[2][4] > seen[0][4] + 20
    print(f"three predicts in one gap, device vs host header: largest relative difference {worst:.3e}")
    assert worst <= TOL, worst
    fl.close()
