"""CPU: the inputs of tests/filters_edges.py qualified against the host header, and the header anchored to oracle/ekf_oracle.py at those inputs.
What tests/test_gpu_filters_edges.py relies on is asserted here without a GPU: every singular case reaches hnet_ekf::invert's zero pivot in the intended
column, the pivoting cases swap rows (often enough, in enough columns), no session of the edge table comes near quat_apply_rotvec's sign flip, and
include/hnet_ekf.h (through tests/cpp/filters_ref.cpp, filters_innov_ref.cpp and ekf_check.cpp) agrees with the numpy restatement on the whole table
within the tolerances tests/test_ekf_cpu.py uses for the same functions."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import filters_edges as fe
import test_ekf_cpu as te
import test_filters_cpu as tc
import test_filters_innov_cpu as ti
from oracle import ekf_oracle

NONE, USED, REJECTED, SINGULAR, SKIPPED = range(5)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("filters_ref") / "filters_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread", "-I", tc.ROOT + "/include",
                    tc.ROOT + "/tests/cpp/filters_ref.cpp", "-o", so], check=True)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def iref(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("filters_innov_ref") / "filters_innov_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread", "-I", tc.ROOT + "/include",
                    tc.ROOT + "/tests/cpp/filters_innov_ref.cpp", "-o", so], check=True)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def sessions():
    return fe.edge_sessions()


def _base(rng, t=fe.T_FRAME):
    import test_gpu_filters as tg
    return tg._state(tc._cabi(), rng, t)


def _net(rng, iters, scale=1.0):
    """network records like the synthetic weights': means of a few pixels, a covariance about `scale` times the identity (px^2), positive definite"""
    net = np.zeros((iters, 72), np.float32)
    for it in range(iters):
        a = rng.standard_normal((8, 8)) * 0.06
        net[it, :8] = rng.standard_normal(8) * 3.0
        net[it, 8:] = (scale * (np.eye(8) * (1.0 + 0.1 * rng.standard_normal(8)) + a @ a.T)).astype(np.float32).reshape(-1)
    return net


# ---------------------------------------------------------------------------------------------- the restatement itself
def test_gauss_jordan_agrees_with_numpy_inverse():
    rng = np.random.default_rng(1)
    mats = [fe.pivot_s8(p) for p in fe.PIVOT_PERMS]
    mats += [fe.pivot_s8(p) + 10.0 * _net(rng, 1)[0, 8:].astype(float).reshape(8, 8) / fe.F_PIX ** 2 for p in fe.PIVOT_PERMS]
    for _ in range(4):
        a = rng.standard_normal((8, 8))
        mats.append(a @ a.T + np.eye(8) * 1e-3)
    for s in mats:
        inv, _swaps, col = fe.gauss_jordan(s)
        want = np.linalg.inv(s)
        assert col is None and np.abs(inv - want).max() <= 1e-12 * np.linalg.cond(s) * np.abs(want).max()


# ---------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("case", fe.SINGULAR_CASES, ids=[c[0] for c in fe.SINGULAR_CASES])
@pytest.mark.parametrize("iters", [1, 3])
def test_singular_cases_reach_the_zero_pivot_in_the_header(ref, iref, case, iters):
    name, s8, col = case
    assert set(np.unique(np.abs(s8))) <= {0.0, 2.0 ** -10}                   # zeros and powers of two: exact in any IEEE arithmetic
    assert fe.gauss_jordan(s8) == (None, [], col)
    rng = np.random.default_rng(3)
    st = fe.singular_state(_base(rng), rng, s8)
    net = _net(rng, iters)
    assert all(fe.net_cov_is_pd(n) for n in net)
    p = tc._params()
    for k, singular in ((0.0, True), (p.k_net_cov, False)):
        p.k_net_cov = k
        assert (fe.gauss_jordan(fe.s_matrix(st["cov"][0], net[0], k))[2] is not None) == singular
        s = st.copy()
        u = ref.ref_iterated_update(C.c_void_p(s.ctypes.data), C.byref(p), iters, C.c_void_p(net.ctypes.data), 1)
        rec = np.zeros(iters, ti.INNOV)
        s2 = st.copy()
        u2 = iref.innov_ref_iterated_gated(C.c_void_p(s2.ctypes.data), C.byref(p), iters, C.c_void_p(net.ctypes.data), 1, C.c_double(0.0),
                                           C.c_void_p(rec.ctypes.data), None, None)
        assert s.tobytes() == s2.tobytes()
        if singular:
            assert u == u2 == -1 and s.tobytes() == fe.expected_after_singular(st, fe.T_FRAME).tobytes()
            assert list(rec["flag"]) == [SINGULAR] + [SKIPPED] * (iters - 1)
            assert np.isnan(rec["nis"][0]) and np.array_equal(rec["s_diag"][0], np.diag(s8))
            assert np.array_equal(rec["r"][0], net[0, :8].astype(float) / fe.F_PIX - st["offset"][0][:, :2].reshape(8))
            assert not rec["r"][1:].any() and not rec["s_diag"][1:].any() and not rec["nis"][1:].any()
        else:
            assert u == u2 == iters and list(rec["flag"]) == [USED] * iters


def test_a_singular_session_with_imu_intervals_is_not_singular_any_more(ref):
    """why case A has no session with real IMU intervals before the update: one propagation fills the zero offset block"""
    rng = np.random.default_rng(4)
    import test_gpu_filters as tg
    st = fe.singular_state(_base(rng, fe.T_FRAME - 0.0324), rng, fe.SINGULAR_CASES[0][1])
    imu = tg._imu(rng, fe.T_FRAME - 0.0324, 16)
    assert tc._propagate(ref, st, tc._params(), fe.T_FRAME, imu.view(np.float64).reshape(-1, 7)) == 17
    s = fe.s_matrix(st["cov"][0], np.zeros(72, np.float32), 0.0)
    assert fe.gauss_jordan(s)[2] is None and np.diag(s).min() > 0


# ---------------------------------------------------------------------------------------------- B
def test_pivoting_cases_swap_rows():
    cols = set()
    for k in fe.PIVOT_K0:                                                     # k_net_cov = 0: S is the matrix itself
        s8 = fe.pivot_s8(fe.PIVOT_PERMS[k])
        assert np.linalg.eigvalsh(s8).min() > 0
        inv, swaps, col = fe.gauss_jordan(s8)
        assert col is None and len(swaps) >= 5, (k, swaps)
        cols |= set(swaps)
    assert len(cols) >= 7 > fe.MIN_SWAP_COLUMNS, cols
    rng = np.random.default_rng(2)
    for k in range(len(fe.PIVOT_PERMS)):
        if k in fe.PIVOT_K0:
            continue
        for scale in (0.4, 0.5, 0.7, 1.0, 1.0, 1.0, 1.4, 2.0, 2.5):
            s = fe.s_matrix(_cov_of(fe.pivot_s8(fe.PIVOT_PERMS[k])), _net(rng, 1, scale)[0], 10.0)
            assert len(fe.gauss_jordan(s)[1]) >= fe.MIN_SWAPS, (k, scale)


def _cov_of(s8):
    cov = np.zeros((27, 27))
    cov[np.ix_(fe.SEL, fe.SEL)] = s8
    return cov


def test_pivot_states_are_positive_definite_and_hold_the_block_bit_for_bit():
    rng = np.random.default_rng(5)
    for perm in fe.PIVOT_PERMS:
        s8 = fe.pivot_s8(perm)
        st = fe.pivot_state(_base(rng), rng, s8)
        cov = st["cov"][0]
        assert np.array_equal(cov[np.ix_(fe.SEL, fe.SEL)], s8) and np.array_equal(cov, cov.T)
        assert np.linalg.eigvalsh(cov).min() > 0


# ---------------------------------------------------------------------------------------------- C
def _as_dict(rec):
    return {k: np.array(rec[k][0], float) for k in ("p", "q", "v", "ba", "bg", "offset", "cov")}


def _select(ref, sess):
    _capi = tc._cabi()
    r = np.ascontiguousarray(sess["imu"])
    out = np.zeros(len(r) + 2, _capi.IMU_DTYPE)
    t0 = float(sess["st"]["t"][0]) + sess["p"].cam_imu_dt
    m = ref.ref_select(C.c_void_p(r.ctypes.data), len(r), C.c_double(t0), C.c_double(fe.T_FRAME + sess["p"].cam_imu_dt), C.c_void_p(out.ctypes.data))
    return out[:m]


def test_edge_table_intervals_angles_and_sign_margin(ref, sessions):
    ang = {}
    for s in sessions:
        st, q, ang[s["id"]] = fe.trace(ref, s)
        plain = s["st"].copy()
        r = np.ascontiguousarray(s["imu"])
        n = ref.ref_propagate_with_imu(C.c_void_p(plain.ctypes.data), C.byref(s["p"]), C.c_double(fe.T_FRAME), C.c_void_p(r.ctypes.data), len(r))
        assert n == len(q) == s["n_int"], s["id"]
        assert st.tobytes() == plain.tobytes(), s["id"]                      # the trace is the header's loop
        assert np.all(np.isfinite(st["cov"])) and np.abs(q[:, 3]).min() >= 100 * fe.R3_MARGIN, (s["id"], np.abs(q[:, 3]).min())
        # the ground plane's distance along the camera axis divides the corner dynamics: well away from zero at both ends
        for x in (s["st"], st):
            dc = (ekf_oracle.ham_quat_2_rot(x["q"][0]) @ (x["p"][0] + np.array(s["p"].i_t_i2c)))[2]
            assert abs(dc) > 0.5, (s["id"], dc)
    assert ang["zero_rate_avg1"] == ang["zero_rate_avg0"] == 0.0             # jr_theta's and propagate_jacobians' zero branches, quat_apply_rotvec's limit
    assert 0.9e-13 < ang["angle_1e-13"] < 1.1e-13 and 0.9e-11 < ang["angle_1e-11"] < 1.1e-11      # either side of jr_theta's 1e-12
    assert abs(ang["rate_35_dt_5ms"] - 0.175) < 1e-6 and ang["rate_35_gap_100ms"] > np.pi
    by = {s["id"]: s for s in sessions}
    assert by["q_w_negative"]["st"]["q"][0][0] < 0 and by["q_random"]["st"]["q"][0][3] < 0
    assert by["window_400"]["n_int"] > 40 and by["cam_imu_dt_launch"]["p"].cam_imu_dt == -0.0148489
    d = np.diag(by["cov_12_orders"]["st"]["cov"][0])
    assert d[12:15].max() / d[0:3].min() == pytest.approx(1e-12) and np.linalg.eigvalsh(by["cov_12_orders"]["st"]["cov"][0]).min() > 0
    dts = np.diff(_select(ref, by["dt_1e-9"])["t"])
    assert (dts < 2e-9).sum() == 8 and (dts > 4e-3).sum() >= 8


def test_header_follows_the_numpy_restatement_over_the_edge_table(ref, sessions):
    """every interval of every session: the header's one-interval propagation (filters_ref on a window of exactly that interval) against
    ekf_oracle.jacobians / propagate_mean / propagate_cov from the same state, at test_ekf_cpu's tolerances (1e-13 on the mean relative to max(1, |x|),
    1e-12 on the covariance); the chain then goes on from the header's state"""
    _capi = tc._cabi()
    worst_m = worst_c = 0.0
    for s in sessions:
        p = s["p"]
        c_R_i, t_i2c = np.array(p.c_R_i).reshape(3, 3), np.array(p.i_t_i2c)
        Q = ekf_oracle.noise_q(p.sigma_w, p.sigma_a, p.sigma_wb, p.sigma_ab)
        sel = _select(ref, s)
        one = tc._params()
        C.memmove(C.byref(one), C.byref(p), C.sizeof(one))
        one.cam_imu_dt = 0.0
        cur = s["st"].copy()
        for k in range(len(sel) - 1):
            a, b = sel[k], sel[k + 1]
            d = _as_dict(cur)
            w1, w2, a1, a2 = a["wm"] - d["bg"], b["wm"] - d["bg"], a["am"] - d["ba"], b["am"] - d["ba"]
            w_hat, a_hat = (0.5 * (w1 + w2), 0.5 * (a1 + a2)) if p.imu_avg else (w2, a2)
            dt = b["t"] - a["t"]
            F, Fw = ekf_oracle.jacobians(d, c_R_i, t_i2c, dt, w_hat, p.gravity_mag)
            want = ekf_oracle.propagate_mean(d, c_R_i, t_i2c, dt, w_hat, a_hat, p.gravity_mag)
            want["cov"] = ekf_oracle.propagate_cov(d["cov"], F, Fw, Q)
            win = np.zeros(3, _capi.IMU_DTYPE)
            win[0], win[1], win[2] = a, b, b
            win[2]["t"] = b["t"] + 1.0
            cur["t"] = a["t"]
            assert ref.ref_propagate_with_imu(C.c_void_p(cur.ctypes.data), C.byref(one), C.c_double(float(b["t"])), C.c_void_p(win.ctypes.data), 3) == 1
            got = _as_dict(cur)
            for f in ("p", "q", "v", "ba", "bg", "offset"):
                e = np.abs(got[f] - want[f]).max() / max(1.0, np.abs(want[f]).max())
                worst_m = max(worst_m, e)
                assert e < 1e-13, (s["id"], k, f, e)
            e = np.abs(got["cov"] - want["cov"]).max() / max(1.0, np.abs(want["cov"]).max())
            worst_c = max(worst_c, e)
            assert e < 1e-12, (s["id"], k, e)
    print(f"header vs numpy restatement over the edge table: mean {worst_m:.3e}, covariance {worst_c:.3e}")


def test_header_update_follows_the_numpy_restatement_after_the_edge_propagations(ref, sessions, tmp_path):
    """hnet_ekf::update (ekf_check) on every propagated state of the table against ekf_oracle.update, at test_ekf_cpu's 1e-11"""
    te._build()
    rng = np.random.default_rng(6)
    cases = []
    for k, s in enumerate(sessions):
        st, _q, _ang = fe.trace(ref, s)
        d = _as_dict(st)
        net = _net(rng, 1)[0].astype(float)
        prop = d["offset"][:, :2].reshape(8).copy()
        cases.append((d, net[:8] + prop * fe.F_PIX, net[8:].reshape(8, 8), prop, s["p"].k_net_cov, k % 2 == 0))
    blob = [np.array([float(len(cases))])]
    for d, mean, ncov, prop, kc, upd in cases:
        blob += [te._flat(d), mean, ncov.reshape(-1), prop, np.array([kc, 1.0 if upd else 0.0])]
    fin, fout = tmp_path / "in.f64", tmp_path / "out.f64"
    np.concatenate(blob).astype("<f8").tofile(fin)
    subprocess.run([te.BIN, str(fin), str(fout)], check=True, timeout=60)
    got = np.fromfile(fout, "<f8").reshape(len(cases), 1 + 2 * te.NSTATE)
    for (d, mean, ncov, prop, kc, upd), g, s in zip(cases, got, sessions):
        want = ekf_oracle.update(d, mean, ncov, prop, kc, upd)
        r1 = te._flat(want)
        assert g[0] == 1.0 and np.abs(g[1:1 + te.NSTATE] - r1).max() < 1e-11 * max(1.0, np.abs(r1).max()), s["id"]
        assert want["q"][3] >= fe.R3_MARGIN, s["id"]
        r2 = te._flat(ekf_oracle.reset_4pt_offset(want))
        assert np.abs(g[1 + te.NSTATE:] - r2).max() < 1e-11 * max(1.0, np.abs(r2).max()), s["id"]


def test_jr_theta_gives_the_identity_on_both_sides_of_its_threshold(tmp_path):
    """F's attitude / gyro-bias block is -dt jr_theta(w dt).  At |w| dt = 1e-13 the header returns the identity outright; at 1e-11 it evaluates
    (1 - cos n) / n^2 and (n - sin n) / n^3, whose numerators are zero in fp64 for any n below about 1e-8, and the block is -dt I to the bit as well.
    So moving the threshold anywhere below that changes no output bit on host or device: no test can tell, and none here pretends to."""
    te._build()
    rng = np.random.default_rng(7)
    st = te._prop_state(rng)
    qd = np.diag(ekf_oracle.noise_q(0.00559017, 0.01118034, 8.94427e-04, 0.04472136))
    dt = 0.002
    ws = [np.array([3e-11, -4e-11, 0.0]), np.array([3e-9, -4e-9, 0.0]), np.array([3e-4, -4e-4, 0.0])]
    blob = [np.array([float(len(ws))])]
    for w in ws:
        blob += [te._flat(st), te.C_R_I.reshape(-1), te.T_I2C, np.array([dt]), w, np.array([0.0, 0.0, 9.81]), qd]
    fin, fout = tmp_path / "in.f64", tmp_path / "out.f64"
    np.concatenate(blob).astype("<f8").tofile(fin)
    subprocess.run([te.BIN, str(fin), str(fout), "jac"], check=True, timeout=60)
    got = np.fromfile(fout, "<f8").reshape(len(ws), 729 + 405 + te.NSTATE)
    blocks = [g[:729].reshape(27, 27)[3:6, 12:15] for g in got]
    assert np.array_equal(blocks[0], -dt * np.eye(3)) and np.array_equal(blocks[1], -dt * np.eye(3))
    assert not np.array_equal(blocks[2], -dt * np.eye(3))                     # (at 1e-6 rad the formula does show)
