"""CPU: the additions of include/hnet_ekf.h that hnet_filters_predict_cov runs.  The convention of OdometryCov::pose_cov is pinned against central
differences of the perturbation update() itself applies (p + dp, quat_apply_rotvec(dtheta, q)), which a left-perturbation Jacobian cannot pass;
odometry_cov_from_state against a numpy restatement; propagate_jacobians_fill on buffers zeroed once against propagate_jacobians as it stood before
the split (kept verbatim in tests/cpp/filters_predict_cov_ref.cpp), byte for byte; the host restatement of the call the GPU tests compare with; the
predict_cov section of the C ABI."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import test_filters_cpu as tc
import test_filters_predict_cpu as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEL = [15 + 3 * (j >> 1) + (j & 1) for j in range(8)]
FRD = [1, 0, 2]                                                 # body = (-y, -x, -z): the two signs of a covariance element cancel
H = 1e-6                                                        # central differences: truncation ~ h^2 |p|, rounding ~ eps |p| / h, both below 1e-9 for |p| <= 10
GATE = 1e-7


def build_ref(so):
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filters_predict_cov_ref.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    vp = C.c_void_p
    L.pcov_ref_odometry_cov.argtypes = [vp, vp]
    L.pcov_ref_odometry.argtypes = [vp, C.c_double, vp]
    L.pcov_ref_predict.argtypes = [vp, vp, C.c_double, vp, C.c_int, vp, vp, vp]
    L.pcov_ref_predict_batch.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp]
    L.pcov_ref_jacobian.argtypes = [vp, vp]
    L.pcov_ref_perturb.argtypes = [vp, vp]
    L.pcov_ref_wpos_rot.argtypes = [vp, vp, vp]
    L.pcov_ref_jacobians3.argtypes = [vp, vp, C.c_double, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    for f in (L.pcov_ref_odometry_cov, L.pcov_ref_odometry, L.pcov_ref_predict, L.pcov_ref_predict_batch, L.pcov_ref_jacobian, L.pcov_ref_perturb,
              L.pcov_ref_wpos_rot, L.pcov_ref_jacobians3):
        f.restype = None
    return L


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return build_ref(str(tmp_path_factory.mktemp("filters_predict_cov_ref") / "filters_predict_cov_ref.so"))


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return pc.build_ref(str(tmp_path_factory.mktemp("filters_predict_ref") / "filters_predict_ref.so"))


def _spd(rng, n=27, scale=0.01):
    a = rng.standard_normal((n, n)) * scale
    return a @ a.T + np.eye(n) * 1e-4


def _attitudes():
    rng = np.random.default_rng(21)
    qs = [q / np.linalg.norm(q) for q in rng.standard_normal((10, 4))]
    qs += [np.array([-abs(q[0]), q[1], q[2], q[3]]) for q in qs[:3]]                     # w < 0
    qs += [np.array([0.0, 1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0, 0.0]), np.array([0.0, 0.0, 0.0, 1.0])]   # the three half turns
    return qs


def _skew(p):
    return np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])


def _rotvec(M):
    """the rotation vector of a rotation matrix close to the identity"""
    v = 0.5 * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    s = np.linalg.norm(v)
    return v * (math.asin(s) / s) if s > 0 else v


def _pose(cref, st):
    w, R = np.zeros(3), np.zeros(9)
    cref.pcov_ref_wpos_rot(st.ctypes.data, w.ctypes.data, R.ctypes.data)
    return w, R.reshape(3, 3)


def test_pose_jacobian_is_that_of_updates_own_perturbation(cref):
    rng = np.random.default_rng(22)
    qs = _attitudes()
    assert sum(q[0] < 0 for q in qs) >= 3
    worst = 0.0
    for k, q in enumerate(qs):
        st = tc._state(rng)
        p = rng.standard_normal(3)
        st["q"], st["p"] = q, p / np.linalg.norm(p) * (10.0 if k % 4 == 0 else rng.uniform(0.1, 10.0))
        J = np.zeros(36)
        cref.pcov_ref_jacobian(st.ctypes.data, J.ctypes.data)
        J = J.reshape(6, 6)
        _, R = _pose(cref, st)
        num = np.zeros((6, 6))
        for c in range(6):
            f = []
            for sgn in (1.0, -1.0):
                s2 = st.copy()
                dx = np.zeros(6)
                dx[c] = sgn * H
                cref.pcov_ref_perturb(s2.ctypes.data, dx.ctypes.data)
                w2, R2 = _pose(cref, s2)
                f.append(np.concatenate([w2, _rotvec(R2 @ R.T)]))
            num[:, c] = (f[0] - f[1]) / (2 * H)
        err = float(np.abs(num - J).max())
        worst = max(worst, err)
        assert err <= GATE, (k, q, err)
        # the Jacobian of an attitude error applied on the LEFT (R <- Exp(dtheta) R) must miss the same gate by orders of magnitude
        pw = R @ st["p"][0]
        J_left = np.block([[R, -_skew(pw)], [np.zeros((3, 3)), np.eye(3)]])
        err_left = float(np.abs(num - J_left).max())
        assert err_left > 1e4 * GATE, (k, q, err_left)
    print(f"pose Jacobian against central differences: largest difference {worst:.3e} (gate {GATE:.0e})")


def test_odometry_cov_matches_numpy(cref):
    _capi = tc._cabi()
    rng = np.random.default_rng(23)
    for k, q in enumerate(_attitudes()):
        st = tc._state(rng)
        st["q"], st["p"], st["cov"] = q, rng.standard_normal(3) * 3.0, _spd(rng)
        out = np.zeros(1, _capi.ODOMETRY_COV_DTYPE)
        cref.pcov_ref_odometry_cov(st.ctypes.data, out.ctypes.data)
        o, P = out[0], st["cov"][0]
        R = pc.np_ham_quat_2_rot(q)
        J = np.block([[R, -R @ _skew(st["p"][0])], [np.zeros((3, 3)), R]])
        want = J @ P[:6, :6] @ J.T
        assert np.abs(o["pose_cov"] - want).max() <= 1e-12 * np.abs(want).max(), k
        assert o["body_pos_cov"].tobytes() == np.ascontiguousarray(o["pose_cov"][:3, :3][np.ix_(FRD, FRD)]).tobytes()
        assert o["body_vel_cov"].tobytes() == np.ascontiguousarray(P[6:9, 6:9][np.ix_(FRD, FRD)]).tobytes()
        assert o["prior_cov_px"].tobytes() == np.ascontiguousarray((159.5 * 159.5) * P[np.ix_(SEL, SEL)]).tobytes()
        # the signed permutation written out: S C S^T with S = -[e_y e_x e_z] is the same matrix
        S = -np.eye(3)[FRD]
        assert np.array_equal(o["body_pos_cov"], S @ o["pose_cov"][:3, :3] @ S.T)
        assert np.abs(o["pose_cov"] - o["pose_cov"].T).max() <= 1e-15 * np.abs(o["pose_cov"]).max()
        assert np.linalg.eigvalsh(0.5 * (o["pose_cov"] + o["pose_cov"].T)).min() > 0.0


def _jac3(cref, st, p, dt, w_hat, reps=2):
    bufs = [np.full(n, np.nan) for n in (729, 405, 729, 405)] + [np.zeros(729), np.zeros(405)]   # a, b: every entry must be written; c: zeroed once
    w = np.ascontiguousarray(w_hat, dtype=np.float64)
    cref.pcov_ref_jacobians3(st.ctypes.data, C.addressof(p), float(dt), w.ctypes.data, reps, *[b.ctypes.data for b in bufs])
    return bufs


def test_fill_on_zeroed_buffers_equals_the_body_before_the_split(cref):
    rng = np.random.default_rng(24)
    p = tc._params()
    cases = [(0.002, None)] * 1000 + [(1e-9, None), (0.1, None), (0.002, np.zeros(3)), (1e-9, np.zeros(3)), (0.1, np.zeros(3))]
    nonzero = None
    for k, (dt, w_hat) in enumerate(cases):
        st = tc._state(rng)
        q = rng.standard_normal(4)
        st["q"], st["p"] = q / np.linalg.norm(q), rng.standard_normal(3) * 2.0
        p.gravity_mag = 9.81 if k % 7 else 1.62
        w = rng.standard_normal(3) * (0.3 if k % 5 else 20.0) if w_hat is None else w_hat
        Fa, Wa, Fb, Wb, Fc, Wc = _jac3(cref, st, p, dt, w, reps=1 + k % 3)
        assert Fa.tobytes() == Fb.tobytes() == Fc.tobytes() and Wa.tobytes() == Wb.tobytes() == Wc.tobytes(), k
        assert np.all(np.isfinite(Fa)) and np.all(np.isfinite(Wa))
        nz = (Fa != 0).tobytes() + (Wa != 0).tobytes()
        if w_hat is None and k < 1000:                          # generic inputs: the entries that are not zero are the same in every interval
            nonzero = nonzero or nz
            assert nz == nonzero, k
    p.gravity_mag = 9.81


@pytest.mark.parametrize("imu_avg", [1, 0])
@pytest.mark.parametrize("intervals", sorted(pc.WINDOWS))
def test_host_predict_cov_is_predict_plus_propagate_with_imu(cref, pref, intervals, imu_avg):
    """the record equals filters_predict_ref's, the full covariance equals propagate_with_imu's, the blocks are odometry_cov_from_state of it"""
    _capi = tc._cabi()
    rng = np.random.default_rng(70 * intervals + imu_avg)
    dt_ci = 0.0013
    t0, t1, n = pc.WINDOWS[intervals]
    r = pc._records(tc._readings(0.002 * np.arange(n or 0), rng))
    p = tc._params(cam_imu_dt=dt_ci)
    p.imu_avg = imu_avg
    st = tc._state(rng)
    q = rng.standard_normal(4)
    st["q"], st["cov"], st["t"] = q / np.linalg.norm(q), _spd(rng), t0 - dt_ci
    rp = r.ctypes.data if len(r) else None
    o, oc, full = np.zeros(1, _capi.ODOMETRY_DTYPE), np.zeros(1, _capi.ODOMETRY_COV_DTYPE), np.zeros((27, 27))
    cref.pcov_ref_predict(st.ctypes.data, C.addressof(p), t1 - dt_ci, rp, len(r), o.ctypes.data, oc.ctypes.data, full.ctypes.data)
    want = np.zeros(1, _capi.ODOMETRY_DTYPE)
    pref.pred_ref_predict(st.ctypes.data, C.addressof(p), t1 - dt_ci, rp, len(r), want.ctypes.data)
    assert o.tobytes() == want.tobytes()
    if n is None:
        assert o["status"][0] == _capi.PRED_WAIT_IMU and not full.any() and not oc.tobytes().strip(b"\0")
        return
    assert o["status"][0] == _capi.PRED_OK and o["intervals"][0] == intervals
    b = st.copy()
    assert pref.pred_ref_full(b.ctypes.data, C.addressof(p), t1 - dt_ci, rp, len(r)) == intervals
    assert full.tobytes() == b["cov"].tobytes()
    assert (full.tobytes() != st["cov"].tobytes()) == (intervals > 0)
    blocks = np.zeros(1, _capi.ODOMETRY_COV_DTYPE)
    cref.pcov_ref_odometry_cov(b.ctypes.data, blocks.ctypes.data)
    assert oc.tobytes() == blocks.tobytes()
    # at or before the state: the state's covariance as it is; the batch form on threads equals the single one
    for tq in (float(st["t"][0]), float(st["t"][0]) - 0.01):
        cref.pcov_ref_predict(st.ctypes.data, C.addressof(p), tq, rp, len(r), o.ctypes.data, oc.ctypes.data, full.ctypes.data)
        cref.pcov_ref_odometry_cov(st.ctypes.data, blocks.ctypes.data)
        assert o["status"][0] == _capi.PRED_AT_STATE and full.tobytes() == st["cov"].tobytes() and oc.tobytes() == blocks.tobytes()
    K = 5
    tq = np.array([t1 - dt_ci, float(st["t"][0]), 10.0, t1 - dt_ci, t0 - dt_ci + 0.001])
    sts, ps = np.repeat(st, K), (type(p) * K)(*([p] * K))
    off = (np.arange(K + 1) * len(r)).astype(np.int64)
    imu = np.ascontiguousarray(np.tile(r, K))
    one = [np.zeros(K, _capi.ODOMETRY_DTYPE), np.zeros(K, _capi.ODOMETRY_COV_DTYPE), np.zeros((K, 27, 27))]
    for i in range(K):
        cref.pcov_ref_predict(st.ctypes.data, C.addressof(p), float(tq[i]), rp, len(r), one[0][i:].ctypes.data, one[1][i:].ctypes.data, one[2][i:].ctypes.data)
    assert one[0]["status"][2] == _capi.PRED_WAIT_IMU
    for T in (1, 4):
        got = [np.zeros(K, _capi.ODOMETRY_DTYPE), np.zeros(K, _capi.ODOMETRY_COV_DTYPE), np.zeros((K, 27, 27))]
        cref.pcov_ref_predict_batch(sts.ctypes.data, ps, K, tq.ctypes.data, imu.ctypes.data, off.ctypes.data, T, *[g.ctypes.data for g in got])
        assert [g.tobytes() for g in got] == [w.tobytes() for w in one]


def test_predict_cov_section_is_declared():
    _capi = tc._cabi()
    header = open(os.path.join(ROOT, "include", "hnet.h")).read()
    for name in ("hnet_filters_predict_cov", "hnet_filters_last_predict_cov_device_ms", "hnet_odometry_cov"):
        assert name in header
    for name in ("hnet_filters_predict_cov", "hnet_filters_last_predict_cov_device_ms"):
        assert name in _capi.SYMBOLS
    assert _capi.ODOMETRY_COV_DTYPE.itemsize == 118 * 8
    ekf = open(os.path.join(ROOT, "include", "hnet_ekf.h")).read()
    for name in ("struct OdometryCov", "odometry_cov_from_state", "propagate_jacobians_fill"):
        assert name in ekf
    L = _capi.lib()
    out, cov = np.zeros(1, _capi.ODOMETRY_DTYPE), np.zeros(1, _capi.ODOMETRY_COV_DTYPE)
    ids, tq = np.zeros(1, np.int32), np.zeros(1)
    assert L.hnet_filters_predict_cov(None, 1, ids.ctypes.data, tq.ctypes.data, out.ctypes.data, cov.ctypes.data, None) == 1
    assert not out.tobytes().strip(b"\0") and not cov.tobytes().strip(b"\0")
    assert math.isnan(L.hnet_filters_last_predict_cov_device_ms(None))
    from cuahn_vio_amd.homography_net import HnetFilters
    assert callable(HnetFilters.predict_cov) and callable(HnetFilters.last_predict_cov_device_ms)
