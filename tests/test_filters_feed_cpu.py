"""CPU: the cold-start half of include/hnet_ekf.h that the fed filters run (initialize_with_imu, initialize_cov, the two retention rules, select_span),
against a numpy restatement of InertialInitializer.cpp:163-279 and StateHelper.cpp:35-61 written here, and the fed-filters section of the C ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAVITY = 9.81
THRESH = 0.5


@pytest.fixture(scope="module")
def fref(tmp_path_factory):
    return build_ref(str(tmp_path_factory.mktemp("filters_feed_ref") / "filters_feed_ref.so"))


def build_ref(so):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filters_feed_ref.cpp"), "-o", so], check=True)
    return C.CDLL(so)


def _cabi():
    from cuahn_vio_amd import _capi
    return _capi


def imu_records(r):
    return np.ascontiguousarray(np.asarray(r, dtype=np.float64).reshape(-1, 7)).view(_cabi().IMU_DTYPE).reshape(-1)


# ---- the streams: [n][7] = t, wm, am at 200 Hz.  A tilted, still IMU measures R^T (0, 0, g) + bias + a little noise; a jerk adds a few m/s^2 ----
def _still(ts, rng, tilt, noise=0.01):
    r = np.zeros((len(ts), 7))
    r[:, 0] = ts
    cr, sr, cp, sp = np.cos(tilt[0]), np.sin(tilt[0]), np.cos(tilt[1]), np.sin(tilt[1])
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    g_i = (Ry @ Rx).T @ np.array([0.0, 0.0, GRAVITY])
    r[:, 1:4] = np.array([0.003, -0.002, 0.001]) + 0.001 * rng.standard_normal((len(ts), 3))
    r[:, 4:7] = g_i + np.array([0.02, -0.03, 0.05]) + noise * rng.standard_normal((len(ts), 3))
    return r


def _jerk(r, t_from, rng, amp=3.0):
    m = r[:, 0] > t_from
    r[m, 4:7] += amp * rng.standard_normal((int(m.sum()), 3))
    r[m, 1:4] += 0.3 * rng.standard_normal((int(m.sum()), 3))
    return r


def stream(kind, seed, t_end=3.0, t_start=0.0):
    """kind -> (readings, wait_for_jerk, expected decision).  The newest reading is at t_end; windows are 1 s (the default)."""
    rng = np.random.default_rng(seed)
    tilt = rng.uniform(-0.4, 0.4, 2)
    ts = t_start + np.arange(int(round((t_end - t_start) * 200)) + 1) / 200.0
    if kind == "still_then_jerk":
        return _jerk(_still(ts, rng, tilt), t_end - 1.0, rng), 1, True
    if kind == "always_moving":
        return _jerk(_still(ts, rng, tilt), -1.0, rng), 1, False
    if kind == "never_moving":
        return _still(ts, rng, tilt), 1, False
    if kind == "never_moving_no_wait":
        return _still(ts, rng, tilt), 0, True
    if kind == "too_short":                                   # 1.5 s of readings: below two windows
        return _jerk(_still(ts[ts >= t_end - 1.5], rng, tilt), t_end - 1.0, rng), 1, False
    if kind == "empty_window":                                # nothing in (newest - 2, newest - 1]
        keep = (ts <= t_end - 2.0) | (ts > t_end - 1.0)
        return _jerk(_still(ts[keep], rng, tilt), t_end - 1.0, rng), 1, False
    raise KeyError(kind)


KINDS = ["still_then_jerk", "always_moving", "never_moving", "never_moving_no_wait", "too_short", "empty_window"]


# ---- numpy restatement of InertialInitializer.cpp:28-38 (retention) and :163-279 ----
def np_trim_init(r, w):
    k = 0
    while k < len(r) and r[k, 0] < r[-1, 0] - 3 * w:
        k += 1
    return r[k:]


def np_windows(r, w):
    newest = r[-1, 0]
    w10 = [d for d in r if newest - 1 * w < d[0] <= newest - 0 * w]
    w21 = [d for d in r if newest - 2 * w < d[0] <= newest - 1 * w]
    return w10, w21


def np_deviation(win):
    avg = np.zeros(3)
    for d in win:
        avg = avg + d[4:7]
    avg = avg / len(win)
    var = 0.0
    for d in win:
        e = d[4:7] - avg
        var += e[0] * e[0] + e[1] * e[1] + e[2] * e[2]
    with np.errstate(invalid="ignore", divide="ignore"):
        return avg, np.sqrt(np.float64(var) / np.float64(len(win) - 1))


def np_initialize(r, w, thresh, height, wait):
    """-> None (refused) or dict(t, p, q, v, ba, bg) and the two deviations"""
    if len(r) < 2 or r[-1, 0] - r[0, 0] < 2 * w:
        return None, None
    w10, w21 = np_windows(r, w)
    if not w10 or not w21:
        return None, None
    _, dev10 = np_deviation(w10)
    a_avg, dev21 = np_deviation(w21)
    w_avg = np.zeros(3)
    for d in w21:
        w_avg = w_avg + d[1:4]
    w_avg = w_avg / len(w21)
    if (dev10 < thresh and wait) or (dev21 > thresh and wait):
        return None, (dev10, dev21)
    z = a_avg / np.sqrt(a_avg[0] * a_avg[0] + a_avg[1] * a_avg[1] + a_avg[2] * a_avg[2])
    e1 = np.array([1.0, 0.0, 0.0])
    x = e1 - np.outer(z, z) @ e1
    x = x / np.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
    y = np.array([z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]])
    Ro = np.stack([x, y, z], axis=1)
    rot = Ro.T
    q = np.zeros(4)
    q[0] = 0.5 * np.sqrt(1 + (rot[0, 0] + rot[1, 1] + rot[2, 2]))
    q[1] = (rot[2, 1] - rot[1, 2]) / (4 * q[0])
    q[2] = (rot[0, 2] - rot[2, 0]) / (4 * q[0])
    q[3] = (rot[1, 0] - rot[0, 1]) / (4 * q[0])
    q = q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    out = dict(t=w21[-1][0], p=Ro @ np.array([0.0, 0.0, height]), q=q, v=np.zeros(3), ba=a_avg - Ro @ np.array([0.0, 0.0, GRAVITY]), bg=w_avg)
    return out, (dev10, dev21)


def quat_to_rot(q):
    w, x, y, z = q
    v = np.array([x, y, z])
    sk = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return (w * w - v @ v) * np.eye(3) + 2 * np.outer(v, v) + 2 * w * sk


def np_initialize_cov(P, q):
    P = P.copy()
    P[0:2, 0:2] = 0.0
    P[2, 2] = 0.005 * 0.005
    a = (0.5 / 180.0 * 3.14159265) * (0.5 / 180.0 * 3.14159265)
    P[3, 3] = a
    P[4, 4] = a
    P[5, 5] = 0.0
    P[9:12, 9:12] = np.eye(3) * 0.005 * 0.005
    P[12:15, 12:15] = 0.0
    R = quat_to_rot(q)
    P[0:3, 0:3] = R.T @ P[0:3, 0:3] @ R
    P[3:6, 3:6] = R.T @ P[3:6, 3:6] @ R
    return P


def init_params(wait=1, window=1.0, thresh=THRESH, height=0.1):
    p = _cabi().InitParams()
    p.window_time, p.imu_thresh, p.init_height, p.wait_for_jerk = window, thresh, height, wait
    return p


def c_initialize(fref, r, wait, window=1.0, thresh=THRESH, height=0.1, with_cov=True):
    """the header on the readings as the initialiser holds them (three windows): -> state record or None"""
    _capi = _cabi()
    rec = imu_records(r)
    k = fref.feed_ref_trim_init(C.c_void_p(rec.ctypes.data), len(rec), C.c_double(r[-1, 0] if len(r) else 0.0), C.c_double(window)) if len(rec) else 0
    rec = np.ascontiguousarray(rec[k:])
    st = np.zeros(1, _capi.FILTER_STATE_DTYPE)
    ip = init_params(wait, window, thresh, height)
    ok = fref.feed_ref_init(C.c_void_p(rec.ctypes.data), len(rec), C.byref(ip), C.c_double(GRAVITY), C.c_void_p(st.ctypes.data))
    if not ok:
        return None
    if with_cov:
        fref.feed_ref_init_cov(C.c_void_p(st.ctypes.data))
    return st


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_initialize_with_imu_matches_numpy(fref, kind, seed):
    r, wait, expect = stream(kind, seed)
    want, devs = np_initialize(np_trim_init(r, 1.0), 1.0, THRESH, 0.1, wait)
    if devs is not None:                                       # no case turns on rounding: every deviation is a factor 2 away from the threshold
        for d in devs:
            assert d >= 2 * THRESH or d <= THRESH / 2, devs
    assert (want is not None) == expect
    got = c_initialize(fref, r, wait, with_cov=False)
    assert (got is not None) == expect
    if not expect:
        return
    assert got["t"][0] == want["t"]
    for k in ("p", "q", "ba", "bg"):
        assert _rel(got[k][0], want[k]) < 1e-12, (k, got[k][0], want[k])
    assert (got["v"][0] == 0).all() and (got["offset"][0] == 0).all() and (got["cov"][0] == 0).all()
    if kind == "still_then_jerk":
        assert want["t"] == pytest.approx(2.0, abs=1e-9)       # the last reading of the OLDER window


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_initial_mean_properties(fref, seed):
    """what the frame is for, without the restatement: R(q) maps the older window's mean specific force onto +z, ba + Ro g is that mean,
    p has the length init_height and points along it"""
    r, wait, _ = stream("still_then_jerk", seed)
    st = c_initialize(fref, r, wait, height=0.35, with_cov=False)
    w21 = r[(r[:, 0] > 1.0) & (r[:, 0] <= 2.0)]
    a_avg = w21[:, 4:7].mean(axis=0)
    R = quat_to_rot(st["q"][0])                                 # local -> world
    up = R @ a_avg
    assert np.abs(up - np.array([0, 0, np.linalg.norm(a_avg)])).max() < 1e-9 * np.linalg.norm(a_avg)
    Ro = R.T
    assert np.abs(st["ba"][0] + Ro @ np.array([0, 0, GRAVITY]) - a_avg).max() < 1e-12 * GRAVITY
    assert abs(np.linalg.norm(st["p"][0]) - 0.35) < 1e-12
    assert np.abs(R @ st["p"][0] - np.array([0, 0, 0.35])).max() < 1e-12
    assert np.abs(st["bg"][0] - w21[:, 1:4].mean(axis=0)).max() < 1e-15
    assert abs(np.linalg.norm(st["q"][0]) - 1) < 1e-15


def test_one_reading_windows_pass_like_the_reference(fref):
    """a window of one reading has the deviation 0 / 0 = NaN; neither comparison of the reference refuses a NaN, so the stream is accepted"""
    r = np.zeros((3, 7))
    r[:, 0] = [0.0, 1.0, 2.0]
    r[:, 4:7] = [[0.1, 0.2, 9.8], [0.1, 0.3, 9.7], [2.0, 0.1, 9.0]]
    want, devs = np_initialize(r, 1.0, THRESH, 0.1, 1)
    assert np.isnan(devs[0]) and np.isnan(devs[1]) and want is not None
    got = c_initialize(fref, r, 1, with_cov=False)
    assert got is not None and got["t"][0] == 1.0
    assert _rel(got["q"][0], want["q"]) < 1e-12


@pytest.mark.parametrize("seed", [5, 6])
def test_initialize_cov_matches_numpy(fref, seed):
    _capi = _cabi()
    r, wait, _ = stream("still_then_jerk", seed)
    st = c_initialize(fref, r, wait, with_cov=True)
    q = st["q"][0]
    want = np_initialize_cov(np.zeros((27, 27)), q)
    got = st["cov"][0]
    assert np.abs(got - want).max() < 1e-18
    assert (got == got.T).all() or np.abs(got - got.T).max() < 1e-20
    R = quat_to_rot(q)
    world_q = R @ got[3:6, 3:6] @ R.T
    assert abs(world_q[2, 2]) < 1e-20                           # zero yaw variance in the world frame
    assert world_q[0, 0] == pytest.approx((0.5 / 180.0 * 3.14159265) ** 2, rel=1e-12)
    world_p = R @ got[0:3, 0:3] @ R.T
    assert np.abs(world_p[:2, :2]).max() < 1e-20 and world_p[2, 2] == pytest.approx(0.005 ** 2, rel=1e-12)
    assert (got[15:, :] == 0).all() and (got[:, 15:] == 0).all() and (got[6:9, 6:9] == 0).all()
    # entries outside the blocks it sets are left alone (the reference overwrites, it does not clear)
    st2 = np.zeros(1, _capi.FILTER_STATE_DTYPE)
    st2["q"] = q
    st2["cov"][0][6, 7] = 0.25
    st2["cov"][0][0, 2] = 0.5
    fref.feed_ref_init_cov(C.c_void_p(st2.ctypes.data))
    P0 = np.zeros((27, 27))
    P0[6, 7] = 0.25
    P0[0, 2] = 0.5
    assert np.abs(st2["cov"][0] - np_initialize_cov(P0, q)).max() < 1e-16


def test_retention_rules(fref):
    ts = np.arange(0.0, 14.0, 0.01)
    r = np.zeros((len(ts), 7))
    r[:, 0] = ts
    rec = imu_records(r)
    newest = r[-1, 0]
    k = fref.feed_ref_trim_init(C.c_void_p(rec.ctypes.data), len(rec), C.c_double(newest), C.c_double(1.0))
    assert k == int(np.sum(ts < newest - 3.0)) and len(np_trim_init(r, 1.0)) == len(r) - k
    k = fref.feed_ref_trim_prop(C.c_void_p(rec.ctypes.data), len(rec), C.c_double(newest))
    assert k == int(np.sum(newest - ts > 10)) and 0 < k < len(ts)
    assert fref.feed_ref_trim_prop(C.c_void_p(rec.ctypes.data), 0, C.c_double(0.0)) == 0


def test_select_on_the_span_is_select_on_the_history(fref):
    """the device finds the span of the ring that select_imu_readings can touch from two counts (hnet_ekf::select_span) and runs the header's loop
    on it: same output as on the whole history, for the edge cases of test_filters_cpu.py and for random windows over histories with repeated stamps"""
    import test_filters_cpu as t
    _capi = _cabi()

    def both(r, t0, t1):
        rec = imu_records(r)
        a, b = np.zeros(len(rec) + 2, _capi.IMU_DTYPE), np.zeros(len(rec) + 2, _capi.IMU_DTYPE)
        span = (C.c_int * 2)()
        ma = fref.feed_ref_select(C.c_void_p(rec.ctypes.data), len(rec), C.c_double(t0), C.c_double(t1), C.c_void_p(a.ctypes.data))
        mb = fref.feed_ref_select_span(C.c_void_p(rec.ctypes.data), len(rec), C.c_double(t0), C.c_double(t1), C.c_void_p(b.ctypes.data), span)
        assert ma == mb and a[:ma].tobytes() == b[:mb].tobytes(), (t0, t1)
        return ma, span[1]

    for name, (ts, t0, t1) in t.CASES.items():
        both(t._readings(ts, np.random.default_rng(len(name))), t0, t1)
    rng = np.random.default_rng(17)
    shorter = 0
    for _ in range(300):
        n = int(rng.integers(0, 400))
        steps = rng.uniform(0.0, 0.004, n) * (rng.uniform(size=n) > 0.1)          # one stamp in ten repeats
        r = t._readings(np.cumsum(steps), rng)
        t0 = rng.uniform(-0.05, 0.8)
        m, span_len = both(r, t0, t0 + rng.uniform(1e-6, 0.1))
        shorter += span_len < n
    assert shorter > 200                                        # and the span is what makes it cheap


def test_fed_filters_section_is_declared_in_the_header():
    _capi = _cabi()
    header = open(os.path.join(ROOT, "include", "hnet.h")).read()
    for name in ("hnet_filter_default_init_params", "hnet_filters_enable_feed", "hnet_filters_set_init_params", "hnet_filters_feed_imu",
                 "hnet_filters_initialized", "hnet_filters_uninitialize", "hnet_filters_advance", "hnet_filters_last_selection"):
        assert name in header and name in _capi.SYMBOLS
    for name in ("hnet_init_params", "HNET_ADV_STEPPED = 0", "HNET_ADV_WAIT_IMU = 1", "HNET_ADV_WAIT_INIT = 2", "HNET_ADV_INITIALIZED = 3",
                 "HNET_ADV_PROPAGATED = 4", "HNET_ADV_NO_FRAME = 5"):
        assert name in header
    assert (_capi.ADV_STEPPED, _capi.ADV_WAIT_IMU, _capi.ADV_WAIT_INIT, _capi.ADV_INITIALIZED, _capi.ADV_PROPAGATED, _capi.ADV_NO_FRAME) == (0, 1, 2, 3, 4, 5)
    assert C.sizeof(_capi.InitParams) == 32
    ekf = open(os.path.join(ROOT, "include", "hnet_ekf.h")).read()
    for name in ("initialize_with_imu", "initialize_cov", "trim_imu_init", "trim_imu_prop", "select_span", "init_decide", "init_from_stats", "3.14159265"):
        assert name in ekf


def test_fed_filters_calls_reject_null_handles():
    _capi = _cabi()
    L = _capi.lib()
    p = _capi.InitParams()
    L.hnet_filter_default_init_params(C.byref(p))
    assert (p.window_time, p.imu_thresh, p.init_height, p.wait_for_jerk) == (1.0, 0.5, 0.1, 1)
    L.hnet_filter_default_init_params(None)
    ids = np.zeros(1, np.int32)
    off = np.zeros(2, np.int64)
    rd = np.zeros(1, _capi.IMU_DTYPE)
    st = np.zeros(1, _capi.FILTER_STATE_DTYPE)
    status = np.zeros(1, np.int32)
    cnt = C.c_int(7)
    assert L.hnet_filters_enable_feed(None, 64) == 1
    assert L.hnet_filters_set_init_params(None, 0, C.byref(p)) == 1
    assert L.hnet_filters_feed_imu(None, 1, ids.ctypes.data, rd.ctypes.data, off.ctypes.data) == 1
    assert L.hnet_filters_initialized(None, 0) == -1
    assert L.hnet_filters_uninitialize(None, 0) == 1
    assert L.hnet_filters_advance(None, 1, ids.ctypes.data, st.ctypes.data, None, None, status.ctypes.data) == 1
    assert L.hnet_filters_last_selection(None, 0, rd.ctypes.data, 1, C.byref(cnt)) == 1
