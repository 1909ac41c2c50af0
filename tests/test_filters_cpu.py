"""CPU: the IMU half of include/hnet_ekf.h that hnet_filters runs (select_imu_readings, interpolate_data, the corrected inputs of an
interval, propagate_with_imu), against a numpy restatement of Propagator.cpp:28-204 written here, and the filters section of the C ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("filters_ref") / "filters_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filters_ref.cpp"), "-o", so], check=True)
    return C.CDLL(so)


def _cabi():
    from cuahn_vio_amd import _capi
    return _capi


# ---- numpy restatement of Propagator.h:179-190 and Propagator.cpp:81-175 ----
def np_interp(a, b, t):
    lam = (t - a[0]) / (b[0] - a[0])
    out = np.empty(7)
    out[0] = t
    out[1:] = (1 - lam) * a[1:] + lam * b[1:]
    return out


def np_select(r, t0, t1):
    out = []
    if len(r) == 0:
        return out
    for i in range(len(r) - 1):
        if r[i + 1][0] > t0 and r[i][0] < t0:
            out.append(np_interp(r[i], r[i + 1], t0))
            continue
        if r[i][0] >= t0 and r[i + 1][0] <= t1:
            out.append(r[i].copy())
            continue
        if r[i + 1][0] > t1:
            if r[i][0] > t1 and i == 0:
                break
            elif r[i][0] > t1:
                out.append(np_interp(r[i - 1], r[i], t1))
            else:
                out.append(r[i].copy())
            if out[-1][0] != t1:
                out.append(np_interp(r[i], r[i + 1], t1))
            break
    i = 0
    while i < len(out) - 1:
        if abs(out[i + 1][0] - out[i][0]) < 1e-12:
            del out[i]
        else:
            i += 1
    return out


def _readings(ts, rng):
    r = np.zeros((len(ts), 7))
    r[:, 0] = ts
    r[:, 1:] = rng.standard_normal((len(ts), 6))
    return r


def _c_select(ref, r, t0, t1):
    _capi = _cabi()
    a = np.ascontiguousarray(np.asarray(r, dtype=np.float64).reshape(-1, 7)).view(_capi.IMU_DTYPE).reshape(-1)
    out = np.zeros(len(a) + 2, _capi.IMU_DTYPE)
    m = ref.ref_select(C.c_void_p(a.ctypes.data), len(a), C.c_double(t0), C.c_double(t1), C.c_void_p(out.ctypes.data))
    return out[:m].view(np.float64).reshape(m, 7)


CASES = {
    "inside": (np.arange(0.0, 0.0401, 0.002), 0.0, 0.032),                     # readings on both ends of the window and beyond
    "split_both_ends": (np.arange(0.0, 0.05, 0.002), 0.0031, 0.0317),
    "reading_on_t1": (np.arange(25) * 0.002, 0.0031, 10 * 0.002),
    "last_reading_on_t1": (np.arange(11) * 0.002, 0.0031, 10 * 0.002),
    "reading_on_t0": (np.arange(0.0, 0.05, 0.002), 0.004, 0.0317),
    "imu_slower_than_camera": (np.array([0.0, 0.1, 0.2]), 0.03, 0.063),
    "all_after_t1": (np.array([0.5, 0.6, 0.7]), 0.03, 0.063),             # the low-rate break at i == 0
    "duplicated_stamps": (np.array([0.0, 0.002, 0.004, 0.004, 0.006, 0.006, 0.006, 0.008, 0.010]), 0.001, 0.0075),
    "near_duplicate_at_t0": (np.array([0.0, 0.002, 0.002 + 1e-13, 0.004, 0.006]), 0.002, 0.005),
    "no_readings": (np.zeros(0), 0.0, 0.01),
    "one_reading": (np.array([0.005]), 0.0, 0.01),
    "all_before_t0": (np.array([0.0, 0.001, 0.002]), 0.01, 0.02),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_select_imu_readings_matches_numpy(ref, name):
    ts, t0, t1 = CASES[name]
    r = _readings(ts, np.random.default_rng(len(name)))
    want = np_select(list(r), t0, t1)
    got = _c_select(ref, r, t0, t1)
    assert got.shape[0] == len(want), (got[:, 0], [w[0] for w in want])
    if want:
        np.testing.assert_allclose(got, np.array(want), rtol=0, atol=1e-15)
    if name in ("split_both_ends", "reading_on_t0"):
        assert got[0, 0] == t0 and got[-1, 0] == t1
    if name == "reading_on_t1":                    # the reading on t1 ends the list, no interpolated copy of it
        assert got[-1, 0] == t1 and got[-2, 0] < t1
    if name == "last_reading_on_t1":               # the reference's loop never reaches a LAST reading that sits on t1: one interval short
        assert got[-1, 0] < t1
    if name == "imu_slower_than_camera":
        assert got.shape[0] == 2 and got[0, 0] == t0 and got[1, 0] == t1
    if name in ("all_after_t1", "no_readings", "one_reading", "all_before_t0"):
        assert got.shape[0] < 2
    if name == "duplicated_stamps":
        assert np.all(np.diff(got[:, 0]) >= 1e-12)


def _state(rng=None):
    _capi = _cabi()
    st = np.zeros(1, _capi.FILTER_STATE_DTYPE)
    st["q"] = [1.0, 0.0, 0.0, 0.0]
    st["p"] = [0.0, 0.0, -1.5]
    st["cov"] = np.eye(27) * 1e-4
    if rng is not None:
        st["ba"] = rng.standard_normal(3) * 0.05
        st["bg"] = rng.standard_normal(3) * 0.01
        st["v"] = rng.standard_normal(3) * 0.5
        st["offset"] = rng.standard_normal((4, 3)) * 0.01
    return st


def test_interval_inputs_subtract_biases_and_average(ref):
    _capi = _cabi()
    rng = np.random.default_rng(3)
    st = _state(rng)
    a, b = _readings([0.010, 0.012], rng)
    ia = a.view(_capi.IMU_DTYPE).copy()
    ib = b.view(_capi.IMU_DTYPE).copy()
    w, acc, dt = np.zeros(3), np.zeros(3), C.c_double()
    for avg in (1, 0):
        ref.ref_interval_inputs(C.c_void_p(st.ctypes.data), C.c_void_p(ia.ctypes.data), C.c_void_p(ib.ctypes.data), avg,
                                C.c_void_p(w.ctypes.data), C.c_void_p(acc.ctypes.data), C.byref(dt))
        bg, ba = st["bg"][0], st["ba"][0]
        ww = 0.5 * ((a[1:4] - bg) + (b[1:4] - bg)) if avg else b[1:4] - bg
        aa = 0.5 * ((a[4:7] - ba) + (b[4:7] - ba)) if avg else b[4:7] - ba
        np.testing.assert_allclose(w, ww, rtol=0, atol=1e-15)
        np.testing.assert_allclose(acc, aa, rtol=0, atol=1e-15)
        assert abs(dt.value - 0.002) < 1e-15


def _params(cam_imu_dt=0.0):
    from cuahn_vio_amd.homography_net import HnetFilters
    p = HnetFilters.default_params()
    p.cam_imu_dt = cam_imu_dt
    return p


def _propagate(ref, st, p, t_frame, r):
    _capi = _cabi()
    a = np.ascontiguousarray(np.asarray(r, dtype=np.float64).reshape(-1, 7)).view(_capi.IMU_DTYPE).reshape(-1)
    return ref.ref_propagate_with_imu(C.c_void_p(st.ctypes.data), C.byref(p), C.c_double(t_frame), C.c_void_p(a.ctypes.data), len(a))


def test_propagate_with_imu_intervals_time_and_refusal(ref):
    rng = np.random.default_rng(5)
    p = _params()
    r = _readings(np.arange(0.0, 0.1, 0.002), rng) * [1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1]
    st = _state(rng)
    st["t"] = 0.0031
    n = _propagate(ref, st, p, 0.0317, r)
    assert n == len(np_select(list(r), 0.0031, 0.0317)) - 1 and float(st["t"][0]) == 0.0317
    assert np.all(np.isfinite(st["cov"])) and not np.array_equal(st["cov"], np.eye(27) * 1e-4)
    before = st.copy()
    assert _propagate(ref, st, p, 0.0317, r) == -1 and st.tobytes() == before.tobytes()       # t_frame == t: refused
    assert _propagate(ref, st, p, 0.0300, r) == -1 and st.tobytes() == before.tobytes()       # backwards: refused
    # fewer than two readings: no interval, the state still moves to t_frame (Propagator.cpp:75)
    assert _propagate(ref, st, p, 0.5, np.zeros((0, 7))) == 0
    assert float(st["t"][0]) == 0.5 and np.array_equal(st["cov"], before["cov"]) and np.array_equal(st["p"], before["p"])
    # the camera-IMU offset shifts the window: readings in IMU time [t + dt, t_frame + dt]
    p2 = _params(cam_imu_dt=0.01)
    st2 = _state(rng)
    st2["t"] = 0.0031
    assert _propagate(ref, st2, p2, 0.0317, r) == len(np_select(list(r), 0.0131, 0.0417)) - 1


def test_propagate_with_imu_converges_to_fine_integration(ref):
    """a smooth motion sampled at 16, 64, 256 and 2048 readings over one frame: the coarse results approach the finest one"""
    p = _params()
    T = 0.064

    def motion(n):
        ts = np.linspace(0.0, T, n + 1)
        r = np.zeros((n + 1, 7))
        r[:, 0] = ts
        r[:, 1] = 0.8 * np.sin(20 * ts)
        r[:, 2] = 0.5 * np.cos(15 * ts)
        r[:, 3] = 0.3
        r[:, 4] = 2.0 * np.cos(10 * ts)
        r[:, 5] = 0.5
        r[:, 6] = 9.81 + 0.3 * np.sin(12 * ts)
        return r

    def run(n):
        st = _state()
        st["v"] = [1.0, 0.2, 0.0]
        _propagate(ref, st, p, T, motion(n))
        return np.concatenate([st["p"][0], st["v"][0], st["q"][0], st["offset"][0].reshape(-1)])

    fine = run(2048)
    errs = [np.abs(run(n) - fine).max() for n in (16, 64, 256)]
    assert errs[0] > errs[1] > errs[2] and errs[2] < 1e-3, errs        # first order: about 4x per 4x readings
    assert errs[1] < 0.5 * errs[0] and errs[2] < 0.5 * errs[1]


def test_filters_section_is_declared_in_the_header():
    _capi = _cabi()
    header = open(os.path.join(ROOT, "include", "hnet.h")).read()
    for name in ("hnet_create_filters", "hnet_destroy_filters", "hnet_filters_step", "hnet_filters_set_state", "hnet_filters_get_state",
                 "hnet_filters_set_params", "hnet_filter_default_params", "hnet_filters_last_timing", "hnet_filters_last_priors", "hnet_filter_state",
                 "hnet_imu"):
        assert name in header
        if name.startswith("hnet_f") and name not in ("hnet_filter_state",):
            assert name in _capi.SYMBOLS
    assert _capi.FILTER_STATE_DTYPE.itemsize == 758 * 8 and _capi.IMU_DTYPE.itemsize == 7 * 8
    ekf = open(os.path.join(ROOT, "include", "hnet_ekf.h")).read()
    for name in ("struct ImuData", "interpolate_data", "select_imu_readings", "imu_interval_inputs", "propagate_with_imu"):
        assert name in ekf


def test_filters_calls_reject_null_handles():
    _capi = _cabi()
    L = _capi.lib()
    out = C.c_void_p()
    assert L.hnet_create_filters(None, 1, C.byref(out)) == 1 and not out.value
    p = _capi.FilterParams()
    L.hnet_filter_default_params(C.byref(p))
    assert p.k_net_cov == 10.0 and p.imu_avg == 1 and p.gravity_mag == 9.81 and p.cam_imu_dt == 0.0
    R = np.array(p.c_R_i).reshape(3, 3)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6
    st = np.zeros(1, _capi.FILTER_STATE_DTYPE)
    ids = np.zeros(1, np.int32)
    assert L.hnet_filters_set_params(None, 0, C.byref(p)) == 1
    assert L.hnet_filters_set_state(None, 0, st.ctypes.data) == 1
    assert L.hnet_filters_get_state(None, 1, ids.ctypes.data, st.ctypes.data) == 1
    assert L.hnet_filters_step(None, 1, ids.ctypes.data, None, None, None, None, None, None) == 1
    assert L.hnet_filters_last_timing(None, C.byref(_capi.Timing())) == 1
    assert L.hnet_filters_last_priors(None, 1, st.ctypes.data) == 1
    L.hnet_destroy_filters(None)
