"""CPU: the photometric gate of include/hnet_ekf.h (photo_reject, iterated_update_photo_gated) through tests/cpp/filters_photo_gate_ref.cpp: the rule
against a numpy restatement and at its edges, the gate-off path against iterated_update_gated byte for byte, rejections at every iteration, the order of
the two gates, and the stand-alone program tests/cpp/filters_photo_gate_check.cpp under AddressSanitizer + UndefinedBehaviorSanitizer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_filters_innov_cpu as ti

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHOTO = np.dtype([("sum", "<f8"), ("sum_inside", "<f8"), ("n_inside", "<i4"), ("flags", "<i4")])
DEGENERATE, PH_REJECTED = 1, 2
NONE, USED, REJECTED, SINGULAR, SKIPPED = range(5)
NPIX = 71680


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("filters_photo_gate_ref") / "filters_photo_gate_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filters_photo_gate_ref.cpp"), "-o", so], check=True)
    return C.CDLL(so)


def _rec(sum_inside, n_inside, flags=0, extra=0.0):
    r = np.zeros(1, PHOTO)
    r["sum"], r["sum_inside"], r["n_inside"], r["flags"] = sum_inside + extra, sum_inside, n_inside, flags
    return r


def _reject(pref, prior, est, max_ratio, min_inside):
    return pref.photo_gate_ref_reject(C.c_void_p(prior.ctypes.data), C.c_void_p(est.ctypes.data), C.c_double(max_ratio), int(min_inside))


def _rule(prior, est, max_ratio, min_inside):
    """the rule of the issue restated in numpy float64 (products, no quotient)"""
    if not max_ratio > 0:
        return 0
    need = max(int(min_inside), 1)
    if (int(est["flags"][0]) & DEGENERATE) or int(est["n_inside"][0]) < need:
        return 1
    if (int(prior["flags"][0]) & DEGENERATE) or int(prior["n_inside"][0]) < need:
        return 0
    lhs = np.float64(est["sum_inside"][0]) * np.float64(prior["n_inside"][0])
    rhs = (np.float64(max_ratio) * np.float64(prior["sum_inside"][0])) * np.float64(est["n_inside"][0])
    return int(lhs > rhs)


def test_photo_reject_matches_numpy(pref):
    rng = np.random.default_rng(1)
    seen = [0, 0]
    for case in range(4000):
        prior = _rec(rng.uniform(0, 3e6), int(rng.integers(0, NPIX + 1)), int(rng.integers(0, 4) == 0), rng.uniform(0, 1e5))
        est = _rec(rng.uniform(0, 3e6), int(rng.integers(0, NPIX + 1)), int(rng.integers(0, 6) == 0), rng.uniform(0, 1e5))
        if case % 3 == 0:                                                      # near the boundary: the estimate a few ulps around ratio x prior
            ratio = rng.uniform(0.3, 3.0)
            est["n_inside"] = max(int(prior["n_inside"][0]), 1)
            at = ratio * prior["sum_inside"][0]
            est["sum_inside"] = [np.nextafter(at, 0.0), at, np.nextafter(at, np.inf)][(case // 3) % 3]
        else:
            ratio = [0.0, -1.0, 0.5, 1.0, 2.0, 1e30][case % 6]
        mi = int(rng.choice([0, 1, 1000, 40000, NPIX]))
        got, want = _reject(pref, prior, est, ratio, mi), _rule(prior, est, ratio, mi)
        assert got == want, (case, prior, est, ratio, mi)
        seen[got] += 1
    assert min(seen) > 400, seen


def test_photo_reject_edges(pref):
    p, e = _rec(1000.0, 50000), _rec(3000.0, 50000)
    assert _reject(pref, p, e, 2.0, 0) == 1 and _reject(pref, p, e, 4.0, 0) == 0
    for off in (0.0, -1.0, float("nan")):                                      # max_ratio 0 (and below): never, whatever the records say
        assert _reject(pref, p, e, off, 0) == 0
        assert _reject(pref, p, _rec(0.0, 0, DEGENERATE), off, 0) == 0
    # DEGENERATE: an estimate is refused, a prior gives nothing to compare with
    assert _reject(pref, p, _rec(10.0, 50000, DEGENERATE), 1e30, 0) == 1
    assert _reject(pref, _rec(1000.0, 50000, DEGENERATE), e, 2.0, 0) == 0
    assert _reject(pref, _rec(1000.0, 50000, DEGENERATE), _rec(3000.0, 50000, DEGENERATE), 2.0, 0) == 1      # the estimate's test comes first
    # n_inside 0, or below min_inside, on either side
    assert _reject(pref, p, _rec(0.0, 0), 1e30, 0) == 1
    assert _reject(pref, _rec(0.0, 0), e, 2.0, 0) == 0
    assert _reject(pref, p, _rec(3000.0, 49999), 4.0, 50000) == 1 and _reject(pref, p, _rec(3000.0, 50000), 4.0, 50000) == 0
    assert _reject(pref, _rec(1000.0, 49999), e, 2.0, 50000) == 0 and _reject(pref, _rec(1000.0, 50000), e, 2.0, 50000) == 1
    assert _reject(pref, p, _rec(3000.0, 1), 1e30, 0) == 0 and _reject(pref, p, _rec(3000.0, 1), 1e30, 1) == 0 and _reject(pref, p, _rec(3000.0, 1), 1e30, 2) == 1
    # NaN sums do not reject
    assert _reject(pref, p, _rec(float("nan"), 50000), 2.0, 0) == 0
    assert _reject(pref, _rec(float("nan"), 50000), e, 2.0, 0) == 0
    # exact equality of the two products: "exceeds" is strict.  3 x 1000 x 40000 = 3000 x 40000 ... with different pixel counts on either side
    p2, e2 = _rec(1024.0, 40000), _rec(1536.0, 20000)                          # 1536 x 40000 = (3 x 1024) x 20000 exactly
    assert _reject(pref, p2, e2, 3.0, 0) == 0
    assert _reject(pref, p2, _rec(np.nextafter(1536.0, np.inf), 20000), 3.0, 0) == 1
    assert _reject(pref, p2, e2, np.nextafter(3.0, 0.0), 0) == 1
    # the REJECTED bit of a record plays no part in the rule
    assert _reject(pref, p, _rec(10.0, 50000, PH_REJECTED), 2.0, 0) == 0


def _photo(pref, st, p, net, gate, max_nis, script, max_ratio, min_inside=0):
    s = st.copy()
    iters = len(net)
    nn = np.ascontiguousarray(net, dtype=np.float32)
    sc = np.ascontiguousarray(script)
    assert sc.shape == (1 + iters,)
    rec, prec = np.zeros(iters, ti.INNOV), np.zeros(1 + iters, PHOTO)
    calls, pcalls = C.c_int(0), C.c_int(0)
    offs = np.full((1 + iters, 8), np.nan)
    u = pref.photo_gate_ref_iterated(C.c_void_p(s.ctypes.data), C.byref(p), iters, C.c_void_p(nn.ctypes.data), int(gate), C.c_double(max_nis),
                                     C.c_void_p(sc.ctypes.data), C.c_double(max_ratio), int(min_inside), C.c_void_p(rec.ctypes.data),
                                     C.c_void_p(prec.ctypes.data), C.byref(calls), C.byref(pcalls), C.c_void_p(offs.ctypes.data))
    return s, u, rec, prec, calls.value, pcalls.value, offs


def _nis(pref, st, p, net, gate, max_nis):
    s = st.copy()
    nn = np.ascontiguousarray(net, dtype=np.float32)
    rec = np.zeros(len(net), ti.INNOV)
    calls = C.c_int(0)
    u = pref.photo_gate_ref_iterated_nis(C.c_void_p(s.ctypes.data), C.byref(p), len(net), C.c_void_p(nn.ctypes.data), int(gate), C.c_double(max_nis),
                                         C.c_void_p(rec.ctypes.data), C.byref(calls))
    return s, u, rec, calls.value


def _script(ratios, prior_sum=1000.0, n=50000):
    """records whose estimate / prior ratio at iteration it is ratios[it]"""
    return np.concatenate([_rec(prior_sum, n, extra=7.0)] + [_rec(prior_sum * r, n, extra=9.0) for r in ratios])


@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("gate", [1, 0])
def test_gate_off_is_iterated_update_gated(pref, iters, gate):
    """max_ratio <= 0: state, return value, innovation records and the network's calls are iterated_update_gated's, byte for byte, with and without a NIS
    gate that rejects; the photometric callable is never called and no record is formed"""
    rng = np.random.default_rng(100 * iters + gate)
    p = ti._params()
    for max_ratio in (0.0, -2.0):
        st = ti._state(rng)
        net = np.stack([ti._net(rng, st, 4.0) for _ in range(iters)])
        _, _, r0, _ = _nis(pref, st, p, net, gate, 0.0)
        for max_nis in (0.0, 0.5 * float(r0["nis"].max()) if gate else 1.0):
            a, ua, ra, ca = _nis(pref, st, p, net, gate, max_nis)
            b, ub, rb, prec, cb, pc, _ = _photo(pref, st, p, net, gate, max_nis, _script([100.0] * iters), max_ratio)
            assert a.tobytes() == b.tobytes() and ua == ub and ra.tobytes() == rb.tobytes() and ca == cb == iters
            assert pc == 0 and prec.tobytes() == np.zeros(1 + iters, PHOTO).tobytes()
        assert a.tobytes() != st.tobytes()


def test_gate_that_passes_changes_nothing_but_forms_records(pref):
    rng = np.random.default_rng(7)
    p = ti._params()
    st = ti._state(rng)
    net = np.stack([ti._net(rng, st, 4.0) for _ in range(3)])
    sc = _script([0.4, 1.9, 2.0])
    a, ua, ra, _ = _nis(pref, st, p, net, 1, 0.0)
    b, ub, rb, prec, calls, pc, offs = _photo(pref, st, p, net, 1, 0.0, sc, 2.0)        # 2.0 x prior is AT the gate: not exceeded
    assert a.tobytes() == b.tobytes() and ua == ub == 3 and ra.tobytes() == rb.tobytes() and calls == 3 and pc == 4
    assert prec.tobytes() == sc.tobytes()
    # the callable is handed iteration 0's prior in fp32 and every forward's mean
    prior0 = (st["offset"][0][:, :2].reshape(8) * ti.F).astype(np.float32).astype(np.float64)
    assert np.array_equal(offs[0], prior0) and np.array_equal(offs[1:], net[:, :8].astype(np.float64))
    # the reference gate closed: the prior's record is still formed, nothing is judged
    c, uc, rc, prec_c, _, pcc, _ = _photo(pref, st, p, net, 0, 0.0, _script([100.0] * 3), 2.0)
    assert uc == 0 and list(rc["flag"]) == [NONE] * 3 and pcc == 1 and prec_c[0].tobytes() == sc[0].tobytes() and not prec_c["flags"].any()


@pytest.mark.parametrize("at", [0, 1, 2])
def test_rejection_at_each_iteration(pref, at):
    """I = 3, the estimate of iteration `at` explains the pair worse than max_ratio x the prior: updates 0 .. at - 1 stay, the rest are skipped, the network
    runs 3 times and the offsets are reset; the state is the one a NIS rejection at the same iteration leaves (the first `at` updates, none of them the
    last iteration's, then the reset)"""
    rng = np.random.default_rng(50 + at)
    p = ti._params()
    st = ti._state(rng)
    net = np.stack([ti._net(rng, st, 4.0) for _ in range(3)])
    ratios = [0.5, 0.6, 0.7]
    ratios[at] = 2.5
    sc = _script(ratios)
    got, u, rec, prec, calls, pc, _ = _photo(pref, st, p, net, 1, 0.0, sc, 2.0)
    assert u == at and calls == 3 and pc == 2 + at
    assert list(rec["flag"]) == [USED] * at + [SKIPPED] * (3 - at)
    assert list(prec["flags"]) == [0] * (1 + at) + [PH_REJECTED] + [0] * (2 - at)
    want = sc.copy()
    want["flags"][1 + at] |= PH_REJECTED
    want[2 + at:] = np.zeros(1, PHOTO)[0]                                      # never formed
    assert prec.tobytes() == want.tobytes()
    assert not rec["nis"][at:].any() and not rec["r"][at:].any()
    # the same state through the NIS gate alone: a NIS gate that rejects exactly at `at` leaves the same updates applied
    _, _, r0, _ = _nis(pref, st, p, net, 1, 0.0)
    if at == 0:
        closed, uc, _, _ = _nis(pref, st, p, net, 0, 0.0)
        assert uc == 0 and got.tobytes() == closed.tobytes()
    else:
        ung, _, _, _ = _nis(pref, st, p, net[:at + 1], 1, 0.0)
        assert got.tobytes() != ung.tobytes()
        # iterations 0 .. at - 1 of a longer loop (so that none is "the last", which would drop the offset rows), the rest cut off by a NIS gate at `at`
        huge = net.copy()
        huge[at, :8] += 1e4                                                    # the NIS of iteration `at` beyond any gate
        lim = 10.0 * float(r0["nis"].max())
        viaN, un, rn, _ = _nis(pref, st, p, huge, 1, lim)
        assert un == at and list(rn["flag"]) == [USED] * at + [REJECTED] + [SKIPPED] * (2 - at)
        assert got.tobytes() == viaN.tobytes()
    assert np.all(got["offset"] == 0) and np.all(got["cov"][0][15:, :] == 0)


def test_nis_rejection_or_singular_first_leaves_no_photo_bit(pref):
    rng = np.random.default_rng(61)
    p = ti._params()
    st = ti._state(rng)
    net = np.stack([ti._net(rng, st, 3.0), ti._net(rng, st, 80.0), ti._net(rng, st, 3.0)])
    _, _, r0, _ = _nis(pref, st, p, net, 1, 0.0)
    lim = 2 * float(r0["nis"][0])
    assert r0["nis"][1] > 2 * lim
    sc = _script([0.5, 0.5, 9.0])                                              # would be refused at iteration 2
    a, ua, ra, _ = _nis(pref, st, p, net, 1, lim)
    b, ub, rb, prec, _, pc, _ = _photo(pref, st, p, net, 1, lim, sc, 2.0)
    assert list(rb["flag"]) == [USED, REJECTED, SKIPPED] and ua == ub == 1 and a.tobytes() == b.tobytes() and ra.tobytes() == rb.tobytes()
    assert not (prec["flags"] & PH_REJECTED).any() and pc == 3 and not prec[3]["n_inside"]      # (iteration 2 was never judged)
    # both in the same iteration: the photometric gate comes first, the estimate has no NIS
    sc1 = _script([0.5, 9.0, 0.5])
    _, u1, r1, prec1, _, _, _ = _photo(pref, st, p, net, 1, lim, sc1, 2.0)
    assert u1 == 1 and list(r1["flag"]) == [USED, SKIPPED, SKIPPED] and list(prec1["flags"]) == [0, 0, PH_REJECTED, 0]
    # singular S at iteration 0 (zero P, zero network covariance): the loop ends there
    zs = st.copy()
    zs["cov"] = 0.0
    zn = net.copy()
    zn[:, 8:] = 0.0
    _, uz, rz, precz, cz, pcz, _ = _photo(pref, zs, p, zn, 1, 0.0, _script([0.5, 9.0, 9.0]), 2.0)
    assert uz == -1 and list(rz["flag"]) == [SINGULAR, SKIPPED, SKIPPED] and cz == 1 and pcz == 2 and not (precz["flags"] & PH_REJECTED).any()


def test_degenerate_and_min_inside_in_the_loop(pref):
    rng = np.random.default_rng(71)
    p = ti._params()
    st = ti._state(rng)
    net = np.stack([ti._net(rng, st, 4.0) for _ in range(2)])
    sc = _script([0.5, 0.5])
    sc[2]["flags"] = DEGENERATE
    sc[2]["n_inside"] = 0
    _, u, rec, prec, _, _, _ = _photo(pref, st, p, net, 1, 0.0, sc, 1e30)
    assert u == 1 and list(rec["flag"]) == [USED, SKIPPED] and list(prec["flags"]) == [0, 0, DEGENERATE | PH_REJECTED]
    sc = _script([0.5, 0.5])
    sc[1]["n_inside"] = 49999
    _, u, rec, prec, _, _, _ = _photo(pref, st, p, net, 1, 0.0, sc, 1e30, min_inside=50000)
    assert u == 0 and list(prec["flags"]) == [0, PH_REJECTED, 0]
    _, u, _, prec, _, _, _ = _photo(pref, st, p, net, 1, 0.0, sc, 1e30, min_inside=0)
    assert u == 2 and not prec["flags"].any()


def test_photo_gate_header_under_asan_ubsan(tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    exe = str(tmp_path / "filters_photo_gate_check_san.bin")
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filters_photo_gate_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "photometric gate check: 24 gate-off cases equal, rule and loop ok" in r.stdout, r.stdout
