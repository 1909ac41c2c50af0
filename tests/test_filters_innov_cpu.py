"""CPU: the innovation additions of include/hnet_ekf.h (innovation, iterated_update_gated) through tests/cpp/filters_innov_ref.cpp: the record
against a numpy restatement, the gate-off path against iterated_update bit for bit, the gate rule and its flags, the consistency of the NIS formula,
and the stand-alone program tests/cpp/filters_innov_check.cpp under AddressSanitizer + UndefinedBehaviorSanitizer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = np.dtype([("t", "<f8"), ("p", "<f8", 3), ("q", "<f8", 4), ("v", "<f8", 3), ("ba", "<f8", 3), ("bg", "<f8", 3),
                  ("offset", "<f8", (4, 3)), ("cov", "<f8", (27, 27))])
INNOV = np.dtype([("r", "<f8", 8), ("s_diag", "<f8", 8), ("nis", "<f8"), ("iteration", "<i4"), ("flag", "<i4")])
NONE, USED, REJECTED, SINGULAR, SKIPPED = range(5)
SEL = [15 + 3 * (j // 2) + j % 2 for j in range(8)]
F = 159.5


class Params(C.Structure):
    _fields_ = [("c_R_i", C.c_double * 9), ("i_t_i2c", C.c_double * 3), ("sigma_w", C.c_double), ("sigma_a", C.c_double), ("sigma_wb", C.c_double),
                ("sigma_ab", C.c_double), ("gravity_mag", C.c_double), ("k_net_cov", C.c_double), ("cam_imu_dt", C.c_double), ("imu_avg", C.c_int32)]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("filters_innov_ref") / "filters_innov_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filters_innov_ref.cpp"), "-o", so], check=True)
    return C.CDLL(so)


def _params(k=10.0):
    p = Params()
    p.k_net_cov = k
    return p


def _state(rng):
    st = np.zeros(1, STATE)
    st["t"] = 2.5
    st["q"] = [1.0, 0, 0, 0]
    st["p"] = [0.1, -0.05, -1.2]
    st["v"] = rng.standard_normal(3) * 0.4
    st["offset"] = rng.standard_normal((4, 3)) * 0.005
    a = rng.standard_normal((27, 27)) * 0.01
    st["cov"] = a @ a.T + np.eye(27) * 1e-4
    return st


def _net(rng, st, spread, cov_scale=1.0):
    """a packed record (mean 8 | cov 64, fp32) whose mean lies `spread` pixels around the state's prior"""
    prior = st["offset"][0][:, :2].reshape(8) * F
    a = rng.standard_normal((8, 8)) * 1.5
    c = (a @ a.T + np.eye(8) * 0.5) * cov_scale
    return np.concatenate([prior + rng.standard_normal(8) * spread, c.reshape(64)]).astype(np.float32)


def _gated(ref, st, p, net, gate, max_nis):
    s = st.copy()
    iters = len(net)
    nn = np.ascontiguousarray(net, dtype=np.float32)
    rec = np.zeros(iters, INNOV)
    calls = C.c_int(0)
    u = ref.innov_ref_iterated_gated(C.c_void_p(s.ctypes.data), C.byref(p), iters, C.c_void_p(nn.ctypes.data), int(gate), C.c_double(max_nis),
                                     C.c_void_p(rec.ctypes.data), C.byref(calls), None)
    return s, u, rec, calls.value


def _plain(ref, st, p, net, gate):
    s = st.copy()
    nn = np.ascontiguousarray(net, dtype=np.float32)
    calls = C.c_int(0)
    u = ref.innov_ref_iterated_plain(C.c_void_p(s.ctypes.data), C.byref(p), len(net), C.c_void_p(nn.ctypes.data), int(gate), C.byref(calls))
    return s, u, calls.value


def _innovation(ref, st, mean, cov, prior, k):
    rec = np.zeros(1, INNOV)
    m, c, pr = (np.ascontiguousarray(x, dtype=np.float64) for x in (mean, cov, prior))
    ok = ref.innov_ref_innovation(C.c_void_p(st.ctypes.data), C.c_void_p(m.ctypes.data), C.c_void_p(c.ctypes.data), C.c_void_p(pr.ctypes.data),
                                  C.c_double(k), C.c_void_p(rec.ctypes.data))
    return ok, rec[0]


def test_innovation_matches_numpy(ref):
    rng = np.random.default_rng(1)
    worst = 0.0
    for case in range(40):
        st = _state(rng)
        k = [10.0, 1.0, 37.5][case % 3]
        a = rng.standard_normal((8, 8)) * 2.0
        cov = a @ a.T + np.eye(8) * 0.3
        prior = st["offset"][0][:, :2].reshape(8).copy()
        mean = prior * F + rng.standard_normal(8) * 5.0
        before = st.copy()
        ok, rec = _innovation(ref, st, mean, cov, prior, k)
        assert ok == 1 and rec["flag"] == USED and st.tobytes() == before.tobytes()
        S = st["cov"][0][np.ix_(SEL, SEL)] + k * cov / (F * F)
        r = mean / F - prior
        nis = float(r @ np.linalg.solve(S, r))
        assert np.abs(rec["r"] - r).max() <= 1e-12 * np.abs(r).max()
        assert np.abs(rec["s_diag"] - np.diag(S)).max() <= 1e-12 * np.abs(np.diag(S)).max()
        assert abs(rec["nis"] - nis) <= 1e-10 * nis
        worst = max(worst, abs(rec["nis"] - nis) / nis)
    print(f"innovation vs numpy: worst relative NIS difference {worst:.3g}")


@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("gate", [1, 0])
def test_gate_off_is_iterated_update(ref, iters, gate):
    rng = np.random.default_rng(10 * iters + gate)
    p = _params()
    for max_nis in (0.0, -3.0):
        st = _state(rng)
        net = np.stack([_net(rng, st, 4.0) for _ in range(iters)])
        a, ua, ca = _plain(ref, st, p, net, gate)
        b, ub, rec, cb = _gated(ref, st, p, net, gate, max_nis)
        assert a.tobytes() == b.tobytes() and ua == ub == (iters if gate else 0) and ca == cb == iters
        assert list(rec["flag"]) == [USED if gate else NONE] * iters and list(rec["iteration"]) == list(range(iters))
        assert a.tobytes() != st.tobytes()
        if not gate:
            assert not rec["nis"].any() and not rec["r"].any() and not rec["s_diag"].any()


@pytest.mark.parametrize("iters", [1, 2, 3])
def test_gate_rule_around_first_nis(ref, iters):
    """the later measurements carry a huge covariance, so that their NIS stays far below the first one's: only iteration 0 can be rejected"""
    rng = np.random.default_rng(20 + iters)
    p = _params()
    st = _state(rng)
    net = np.stack([_net(rng, st, 6.0, 1.0 if it == 0 else 1e6) for it in range(iters)])
    ung, uu, rec0, _ = _gated(ref, st, p, net, 1, 0.0)
    nis0 = float(rec0["nis"][0])
    assert uu == iters and nis0 > 0 and np.all(rec0["nis"][1:] < 0.5 * nis0)
    above, ua, ra, ca = _gated(ref, st, p, net, 1, np.nextafter(nis0, np.inf))
    assert above.tobytes() == ung.tobytes() and ua == iters and list(ra["flag"]) == [USED] * iters and ra.tobytes() == rec0.tobytes()
    # a gate AT the NIS does not reject either: the rule is "exceeds"
    at, _, rt, _ = _gated(ref, st, p, net, 1, nis0)
    assert at.tobytes() == ung.tobytes() and rt["flag"][0] == USED
    below, ub, rb, cb = _gated(ref, st, p, net, 1, np.nextafter(nis0, 0.0))
    closed, uc, rc, _ = _gated(ref, st, p, net, 0, 0.0)                       # the reference gate closed: no update + reset
    assert below.tobytes() == closed.tobytes() and ub == 0 and uc == 0 and cb == iters
    assert list(rb["flag"]) == [REJECTED] + [SKIPPED] * (iters - 1) and list(rc["flag"]) == [NONE] * iters
    assert rb["nis"][0] == nis0 and np.array_equal(rb["r"][0], rec0["r"][0]) and not rb["nis"][1:].any()
    assert np.all(below["offset"] == 0) and np.all(below["cov"][0][15:, :] == 0)


def test_rejection_at_iteration_one_keeps_update_zero(ref):
    rng = np.random.default_rng(31)
    p = _params()
    st = _state(rng)
    net = np.stack([_net(rng, st, 3.0), _net(rng, st, 80.0), _net(rng, st, 3.0)])
    _, _, rec0, _ = _gated(ref, st, p, net, 1, 0.0)
    assert rec0["nis"][1] > 4 * rec0["nis"][0]
    got, u, rec, calls = _gated(ref, st, p, net, 1, 2 * float(rec0["nis"][0]))
    assert u == 1 and calls == 3 and list(rec["flag"]) == [USED, REJECTED, SKIPPED] and rec["nis"][1] == rec0["nis"][1]
    # update 0 alone (with the offsets updated: it is not the last iteration), then the reset: two iterations whose second one is gated off
    one, u1, r1, _ = _gated(ref, st, p, net[:2], 1, 2 * float(rec0["nis"][0]))
    assert u1 == 1 and list(r1["flag"]) == [USED, REJECTED] and got.tobytes() == one.tobytes()
    none, _, _, _ = _gated(ref, st, p, net, 0, 0.0)
    assert got.tobytes() != none.tobytes()


def test_singular_and_nan(ref):
    rng = np.random.default_rng(41)
    p = _params()
    st = _state(rng)
    st["cov"] = 0.0
    net = np.stack([_net(rng, st, 3.0) for _ in range(3)])
    net[:, 8:] = 0.0
    a, ua, ca = _plain(ref, st, p, net, 1)
    b, ub, rec, cb = _gated(ref, st, p, net, 1, 15.507)
    assert a.tobytes() == b.tobytes() and ua == 0 and ub == -1 and ca == cb == 1          # iterated_update stops iterating at a singular S
    assert list(rec["flag"]) == [SINGULAR, SKIPPED, SKIPPED] and np.isnan(rec["nis"][0]) and not rec["s_diag"][0].any() and rec["r"][0].any()
    # a NaN NIS of a non-singular S does not reject: the update is applied as iterated_update applies it
    st = _state(rng)
    net = np.stack([_net(rng, st, 3.0)])
    net[0, 3] = np.nan
    a, ua, _ = _plain(ref, st, p, net, 1)
    b, ub, rec, _ = _gated(ref, st, p, net, 1, 15.507)
    assert a.tobytes() == b.tobytes() and ua == ub == 1 and rec["flag"][0] == USED and np.isnan(rec["nis"][0])


def test_nis_is_chi_squared_with_eight_degrees(ref):
    """r ~ N(0, S) for a fixed SPD S: the mean NIS is 8; its standard error over 4000 draws is sqrt(16 / 4000) = 0.063, so 0.4 is more than 6 sigma"""
    rng = np.random.default_rng(5)
    a = rng.standard_normal((8, 8)) * 0.01
    S = a @ a.T + np.eye(8) * 1e-5
    st = np.zeros(1, STATE)
    cov = np.zeros((27, 27))
    cov[np.ix_(SEL, SEL)] = S
    st["cov"] = cov
    L = np.linalg.cholesky(S)
    zero = np.zeros(64)
    prior = np.zeros(8)
    total = 0.0
    for _ in range(4000):
        r = L @ rng.standard_normal(8)
        ok, rec = _innovation(ref, st, r * F, zero, prior, 10.0)
        assert ok == 1
        total += float(rec["nis"])
    mean = total / 4000
    print(f"mean NIS over 4000 draws: {mean:.4f}")
    assert abs(mean - 8.0) <= 0.4


def test_innov_header_under_asan_ubsan(tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    exe = str(tmp_path / "filters_innov_check_san.bin")
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filters_innov_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "24 gate-off cases equal, gate rule ok" in r.stdout, r.stdout


def test_innov_ref_program_prints_records(tmp_path, ref):
    """the program form of filters_innov_ref.cpp on one session: its printed NIS is the library's"""
    rng = np.random.default_rng(7)
    st = _state(rng)
    p = _params()
    net = np.stack([_net(rng, st, 4.0) for _ in range(2)])
    _, _, rec, _ = _gated(ref, st, p, net, 1, 0.0)
    exe, inp = str(tmp_path / "filters_innov_ref.bin"), str(tmp_path / "in.bin")
    subprocess.run(["g++", "-std=c++17", "-O2", "-DINNOV_REF_MAIN", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filters_innov_ref.cpp"), "-o", exe], check=True)
    with open(inp, "wb") as f:
        f.write(np.array([1, 2], np.int32).tobytes() + st.tobytes() + bytes(p) + net.tobytes() + np.array([1], np.int32).tobytes() + np.array([0.0]).tobytes())
    out = subprocess.run([exe, inp], capture_output=True, text=True, check=True, timeout=60).stdout
    m = re.search(r"iteration 1 flag 1 nis (\S+)", out)
    assert "session 0 updates 2" in out and m and float(m.group(1)) == float(rec["nis"][1]), out[:600]
