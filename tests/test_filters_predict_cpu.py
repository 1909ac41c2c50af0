"""CPU: the prediction additions of include/hnet_ekf.h that hnet_filters_predict runs.  propagate_mean_with_imu must leave the mean exactly as
propagate_with_imu does (the same host build, tests/cpp/filters_predict_ref.cpp) and never touch the covariance; odometry_from_state against a numpy
restatement, written here, of what RosVisualizer::publish_state (RosVisualizer.cpp:157-174) and visualize_odometry (:113-144) form from a state;
the predict section of the C ABI."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import test_filters_cpu as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN_FIELDS = ("p", "q", "v", "ba", "bg", "offset")


def build_ref(so):
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filters_predict_ref.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.pred_ref_mean.argtypes = L.pred_ref_full.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int]
    L.pred_ref_odometry.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
    L.pred_ref_predict.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.c_void_p]
    L.pred_ref_predict_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    for f in (L.pred_ref_odometry, L.pred_ref_predict, L.pred_ref_predict_batch):
        f.restype = None
    return L


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return build_ref(str(tmp_path_factory.mktemp("filters_predict_ref") / "filters_predict_ref.so"))


def _records(r):
    _capi = tc._cabi()
    return np.ascontiguousarray(np.asarray(r, dtype=np.float64).reshape(-1, 7)).view(_capi.IMU_DTYPE).reshape(-1)


# windows in IMU time over readings every 2 ms from 0: (t0, t1, the intervals select_imu_readings leaves); None: no readings at all
WINDOWS = {0: (0.0031, 0.0035, None), 1: (0.0031, 0.0035, 50), 2: (0.0031, 0.0055, 50), 40: (0.0031, 0.0811, 50)}


@pytest.mark.parametrize("imu_avg", [1, 0])
@pytest.mark.parametrize("intervals", sorted(WINDOWS))
def test_mean_equals_propagate_with_imu_bit_for_bit(pref, intervals, imu_avg):
    rng = np.random.default_rng(7 * intervals + imu_avg)
    dt_ci = 0.0013
    t0, t1, n = WINDOWS[intervals]
    r = _records(tc._readings(0.002 * np.arange(n or 0), rng))
    p = tc._params(cam_imu_dt=dt_ci)
    p.imu_avg = imu_avg
    st = tc._state(rng)
    q = np.array([1.0, 0, 0, 0]) + rng.standard_normal(4) * 0.1
    st["q"] = q / np.linalg.norm(q)
    st["t"] = t0 - dt_ci
    a, b = st.copy(), st.copy()
    ka = pref.pred_ref_mean(a.ctypes.data, C.addressof(p), t1 - dt_ci, r.ctypes.data if len(r) else None, len(r))
    kb = pref.pred_ref_full(b.ctypes.data, C.addressof(p), t1 - dt_ci, r.ctypes.data if len(r) else None, len(r))
    assert ka == kb == intervals
    for f in ("t",) + MEAN_FIELDS:
        assert a[f].tobytes() == b[f].tobytes(), f
    assert a["cov"].tobytes() == st["cov"].tobytes()                                      # untouched
    if intervals:
        assert b["cov"].tobytes() != st["cov"].tobytes() and a["p"].tobytes() != st["p"].tobytes()
    # refused like propagate_with_imu: a query at or before the state's time, nothing written
    before = a.copy()
    for tq in (float(a["t"][0]), float(a["t"][0]) - 0.01):
        assert pref.pred_ref_mean(a.ctypes.data, C.addressof(p), tq, r.ctypes.data if len(r) else None, len(r)) == -1
        assert a.tobytes() == before.tobytes()


# ---- numpy restatement of the reference's publishers ----
def np_ham_quat_2_rot(q):
    """quat_ops.h:546-550"""
    w, v = q[0], np.asarray(q[1:4])
    sk = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) * (w * w - v @ v) + 2 * np.outer(v, v) + 2 * w * sk


def np_rot2euler(R):
    """RosVisualizer.cpp:303-315"""
    sy = math.sqrt(R[1, 2] * R[1, 2] + R[2, 2] * R[2, 2])
    if sy < 1e-6:
        yaw = 0.0
        roll = math.atan2(-R[2, 1], R[1, 1])
    else:
        yaw = math.atan2(R[0, 1], R[0, 0])
        roll = math.atan2(R[1, 2], R[2, 2])
    return roll, math.atan2(-R[0, 2], sy), yaw, sy


def np_odometry(st, cam_imu_dt):
    i0_R_w = np.array([[0.0, -1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])            # RosVisualizer.cpp:64
    Rot = np_ham_quat_2_rot(st["q"][0])                                                  # PoseCUAHN.h:119 -> HamQuat.h:104
    b_R_w = i0_R_w.T @ Rot.T @ i0_R_w                                                    # :123
    roll, pitch, yaw, sy = np_rot2euler(b_R_w)
    w_pos = Rot @ st["p"][0]                                                             # :132, :171
    v = st["v"][0]
    return {"t_cam": float(st["t"][0]), "t_imu": float(st["t"][0]) + cam_imu_dt, "p": st["p"][0], "q": st["q"][0], "v": v, "w_pos": w_pos,
            "rpy": np.array([roll, pitch, yaw]), "body_pos": np.array([-w_pos[1], -w_pos[0], -w_pos[2]]),   # :134-136
            "body_vel": np.array([-v[1], -v[0], -v[2]]),                                 # :141-144
            "prior_px": st["offset"][0][:, :2].reshape(8) * 159.5}, sy                  # VioManager.cpp:230-234


def _attitudes():
    rng = np.random.default_rng(11)
    qs = [q / np.linalg.norm(q) for q in rng.standard_normal((12, 4))]
    # pitch at 90 degrees: a quarter turn about x times a turn about y keeps the last row of Rot() at (0, 1, 0), so b_R_w(1, 2) = b_R_w(2, 2) = 0
    h, a = math.sqrt(0.5), 0.3
    qs.append(np.array([h * math.cos(a / 2), h * math.cos(a / 2), h * math.sin(a / 2), h * math.sin(a / 2)]))
    return qs


def test_odometry_from_state_matches_numpy(pref):
    _capi = tc._cabi()
    rng = np.random.default_rng(12)
    branches = set()
    for k, q in enumerate(_attitudes()):
        st = tc._state(rng)
        st["q"], st["p"], st["t"] = q, rng.standard_normal(3), 3.0 + k
        out = np.zeros(1, _capi.ODOMETRY_DTYPE)
        pref.pred_ref_odometry(st.ctypes.data, -0.0148489, out.ctypes.data)
        want, sy = np_odometry(st, -0.0148489)
        branches.add(sy < 1e-6)
        for f, w in want.items():
            assert np.abs(out[f][0] - w).max() <= 1e-12, (k, f, out[f][0], w)
        assert out["intervals"][0] == 0 and out["status"][0] == 0
        if sy < 1e-6:
            assert out["rpy"][0][2] == 0.0 and abs(abs(out["rpy"][0][1]) - math.pi / 2) < 1e-9
    assert branches == {True, False}


def test_host_predict_statuses(pref):
    """the host restatement of the call the GPU tests compare with: OK / AT_STATE / WAIT_IMU, and the batch form on threads equals the single one"""
    _capi = tc._cabi()
    rng = np.random.default_rng(13)
    r = _records(tc._readings(0.002 * np.arange(50), rng))
    p = tc._params(cam_imu_dt=0.001)
    st = tc._state(rng)
    st["t"] = 0.0021
    tq = np.array([0.0300, 0.0021, 0.0010, 0.097, 0.2, 0.0511])                          # newest reading 0.098 - 0.001 = 0.097: waits from there on
    want = [_capi.PRED_OK, _capi.PRED_AT_STATE, _capi.PRED_AT_STATE, _capi.PRED_WAIT_IMU, _capi.PRED_WAIT_IMU, _capi.PRED_OK]
    one = np.zeros(len(tq), _capi.ODOMETRY_DTYPE)
    for i, t in enumerate(tq):
        pref.pred_ref_predict(st.ctypes.data, C.addressof(p), t, r.ctypes.data, len(r), one[i:].ctypes.data)
    assert list(one["status"]) == want
    assert list(one["t_cam"]) == [0.0300, 0.0021, 0.0021, 0.0, 0.0, 0.0511] and not one[3:5]["p"].any()
    assert one["intervals"][0] == 15 and one["intervals"][1] == 0
    K = len(tq)
    sts = np.repeat(st, K)
    ps = (type(p) * K)(*([p] * K))
    off = (np.arange(K + 1) * len(r)).astype(np.int64)
    imu = np.ascontiguousarray(np.tile(r, K))
    for T in (1, 4):
        got = np.zeros(K, _capi.ODOMETRY_DTYPE)
        pref.pred_ref_predict_batch(sts.ctypes.data, ps, K, tq.ctypes.data, imu.ctypes.data, off.ctypes.data, T, got.ctypes.data)
        assert got.tobytes() == one.tobytes()


def test_predict_section_is_declared():
    _capi = tc._cabi()
    header = open(os.path.join(ROOT, "include", "hnet.h")).read()
    for name in ("hnet_filters_predict", "hnet_filters_newest_imu_time", "hnet_odometry", "HNET_PRED_OK", "HNET_PRED_NO_STATE", "HNET_PRED_WAIT_IMU",
                 "HNET_PRED_AT_STATE"):
        assert name in header
    for name in ("hnet_filters_predict", "hnet_filters_newest_imu_time"):
        assert name in _capi.SYMBOLS
    assert _capi.ODOMETRY_DTYPE.itemsize == 33 * 8
    assert (_capi.PRED_OK, _capi.PRED_NO_STATE, _capi.PRED_WAIT_IMU, _capi.PRED_AT_STATE) == (0, 1, 2, 3)
    ekf = open(os.path.join(ROOT, "include", "hnet_ekf.h")).read()
    for name in ("propagate_mean_with_imu", "struct Odometry", "odometry_from_state"):
        assert name in ekf
    L = _capi.lib()
    out = np.zeros(1, _capi.ODOMETRY_DTYPE)
    ids, tq = np.zeros(1, np.int32), np.zeros(1)
    assert L.hnet_filters_predict(None, 1, ids.ctypes.data, tq.ctypes.data, out.ctypes.data) == 1 and not out.tobytes().strip(b"\0")
    assert math.isnan(L.hnet_filters_newest_imu_time(None, 0))
