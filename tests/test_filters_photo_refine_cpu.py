"""CPU: the photometric fallback of hnet_filters on the host (include/hnet_photo_refine.h; include/hnet.h hnet_filters_set_photo_refine) through
tests/cpp/filters_photo_refine_ref.cpp: refine_measurement against a numpy float64 restatement on records of the host robust reference, every UNUSABLE
reason on an input of its own, and hnet_ekf::iterated_update_photo_refined with a stub aligner on each of its paths, byte for byte against
iterated_update_photo_gated and against update / reset_4pt_offset called by hand, and the stand-alone program tests/cpp/filters_photo_refine_check.cpp
under AddressSanitizer + UndefinedBehaviorSanitizer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import photo_align_util as U
import photo_robust_util as R
import test_filters_innov_cpu as ti
import test_filters_photo_gate_cpu as tg
from cuahn_vio_amd import _capi

ROOT = U.ROOT
REFINE = _capi.PHOTO_REFINE_DTYPE
ASKED, APPLIED, NIS_REJECTED, S_SINGULAR = 1, 2, 4, 8
BAD_K, STOPPED, NO_STEP, MSE_ABOVE_MAX, NO_FACTOR, NON_FINITE = 16, 32, 64, 128, 256, 512
# measured worst over the records and scales of test_measurement_matches_numpy, max |R - numpy| / max |numpy|: 9.1e-16 (numpy solves the brightness block
# and inverts the Schur complement by LU, the header by Cholesky and Gauss-Jordan; with the 0.05 px floor the difference drops below 1e-17).  Gate: 10 x
MEASURED_R = 9.1e-16


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("filters_photo_refine_ref") / "filters_photo_refine_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filters_photo_refine_ref.cpp"), "-o", so], check=True)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    """level-0 records of the host robust reference at levels = 2, max_iterations = 3 and the trials accepted over both levels: a smooth pair, a stock
    pair from its prior, a pair with the exposure step and the foreign block, and the smooth pair with the model off"""
    rref = R.build_ref(tmp_path_factory.mktemp("photo_robust_ref_for_refine"))
    out = {}
    s1, s2, _ = U.smooth_pair(1, 2.0)
    k1, k2, _, kstart = U.stock_pair(2)
    b1, b2, _, bstart = R.row_pairs("block-1level")
    zero = np.zeros(8, np.float32)
    for name, i1, i2, start, kw in (("smooth", s1, s2, zero, {}), ("stock", k1, k2, kstart, {}), ("spoiled", b1[0], b2[0], bstart[0], {}),
                                    ("model-off", s1, s2, zero, dict(brightness=0, huber_k=0.0))):
        rec, lv = R.ref_run(rref, i1, i2, start, 2, max_iterations=3, **kw)
        out[name] = (rec[0].copy(), int(lv[0]["px"]["accepted"].sum()))
    st1, st2 = U.degenerate_cases()[1][1:3]
    rec, _ = R.ref_run(rref, st1, st2, zero, 1, max_iterations=2, brightness=0, huber_k=0.0)
    out["stripes"] = (rec[0].copy(), 0)
    return out


def _opts(**kw):
    o = _capi.PhotoRefineOpts()
    o.align = R.opts(max_iterations=3)
    o.levels, o.cov_scale, o.sigma_floor_px, o.max_mse = 2, 1.0, 0.05, 0.0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _measure(lib, rec, accepted, o, k=10.0):
    r = np.ascontiguousarray(rec, R.REC).reshape(1)
    out72, r_px, flags = np.full(72, 7.0, np.float32), np.full((8, 8), 7.0), C.c_int32(0)
    ok = lib.photo_refine_ref_measurement(C.c_void_p(r.ctypes.data), int(accepted), C.byref(o), C.c_double(k), C.c_void_p(out72.ctypes.data),
                                          C.c_void_p(r_px.ctypes.data), C.byref(flags))
    return ok, out72, r_px, flags.value


def _numpy_r(rec, o, model_on):
    A = rec["info10"].astype(np.float64)
    info8 = A[:8, :8] - A[:8, 8:] @ np.linalg.solve(A[8:, 8:], A[8:, :8]) if model_on else rec["px"]["info"].astype(np.float64)
    return o.cov_scale * float(rec["px"]["mse"]) * np.linalg.inv(info8) + o.sigma_floor_px ** 2 * np.eye(8)


def test_measurement_matches_numpy(lib, records):
    """R_px = scale * mse * inverse(info8) + floor^2 I against numpy float64 with info8 from numpy's Schur complement, on three records of the host robust
    reference at two scales; R is exactly symmetric with positive Cholesky pivots; the mean is the record's offsets and the packed covariance the fp32 of
    R / k_net_cov; the model-off record takes the px.info path"""
    worst = 0.0
    for name in ("smooth", "stock", "spoiled", "model-off"):
        rec, acc = records[name]
        on = name != "model-off"
        assert acc > 0 and not rec["px"]["flags"] & (U.SINGULAR | U.DEGENERATE | U.FEW_PIXELS), name
        assert bool(rec["info10"][8:].any()) == on
        for o, k in ((_opts(), 10.0), (_opts(cov_scale=4.5, sigma_floor_px=0.0), 37.5)):
            ok, out72, r_px, flags = _measure(lib, rec, acc, o, k)
            assert ok == 1 and flags == 0, (name, flags)
            want = _numpy_r(rec, o, on)
            rel = float(np.abs(r_px - want).max() / np.abs(want).max())
            worst = max(worst, rel)
            print(f"{name}, scale {o.cov_scale}: max |R - numpy| / max |numpy| = {rel:.2e}; sqrt(diag R) = {np.sqrt(np.diag(r_px)).round(4)} px")
            assert rel < 10 * MEASURED_R, (name, rel)
            assert (r_px == r_px.T).all()
            assert (np.diag(np.linalg.cholesky(r_px)) > 0).all()
            assert out72[:8].tobytes() == rec["px"]["offsets_px"].tobytes()
            assert out72[8:].tobytes() == (r_px.reshape(64) / k).astype(np.float32).tobytes()
    print(f"worst relative difference {worst:.2e}")
    # the marginal of the header is what hnet_photo_robust_marginal's test pins: here only that the model-off record copies px.info
    rec, _ = records["model-off"]
    info, grad = np.zeros((8, 8)), np.zeros(8)
    r = np.ascontiguousarray(rec, R.REC).reshape(1)
    assert lib.photo_refine_ref_marginal(C.c_void_p(r.ctypes.data), C.c_void_p(info.ctypes.data), C.c_void_p(grad.ctypes.data)) == 1
    assert info.tobytes() == np.ascontiguousarray(rec["px"]["info"]).tobytes() and grad.tobytes() == rec["px"]["grad"].tobytes()


def _unusable_cases(records):
    good, acc = records["smooth"]
    cases = []
    for fl in (U.SINGULAR, U.DEGENERATE, U.FEW_PIXELS):
        r = good.copy()
        r["px"]["flags"] |= fl
        cases.append((f"flag-{fl}", r, acc, _opts(), 10.0, STOPPED))
    cases.append(("nothing-accepted", good, 0, _opts(), 10.0, NO_STEP))
    stripes = records["stripes"][0].copy()
    stripes["px"]["flags"] = 0                                                 # (the alignment itself says SINGULAR; the rank of info8 must be caught without it)
    cases.append(("stripes", stripes, 1, _opts(), 10.0, NO_FACTOR))
    bad = good.copy()
    bad["info10"][9, 9] = bad["info10"][8, 9] ** 2 / bad["info10"][8, 8] * (1 - 1e-3)       # a negative second pivot of the brightness block
    cases.append(("brightness-block", bad, acc, _opts(), 10.0, NO_FACTOR))
    for k in (0.0, float("nan"), float("inf"), -1.0):
        cases.append((f"k-{k}", good, acc, _opts(), k, BAD_K))
    cases.append(("mse-above-max", good, acc, _opts(max_mse=float(good["px"]["mse"]) * 0.999), 10.0, MSE_ABOVE_MAX))
    huge = good.copy()
    huge["px"]["mse"] = 1e308
    cases.append(("non-finite", huge, acc, _opts(cov_scale=1e10), 10.0, NON_FINITE))
    return cases


def test_every_unusable_reason(lib, records):
    """one input per reason: exactly its bit, and neither out72 nor r_px is written; the same record is usable without the defect"""
    good, acc = records["smooth"]
    assert np.linalg.matrix_rank(records["stripes"][0]["px"]["info"]) < 8 and records["stripes"][0]["px"]["flags"] & U.SINGULAR
    ok, _, _, flags = _measure(lib, good, acc, _opts(max_mse=float(good["px"]["mse"])))    # at the limit: "exceeds" is strict
    assert ok == 1 and flags == 0
    for name, rec, accepted, o, k, bit in _unusable_cases(records):
        ok, out72, r_px, flags = _measure(lib, rec, accepted, o, k)
        assert ok == 0 and flags == bit, (name, flags)
        assert (out72 == 7.0).all() and (r_px == 7.0).all(), name


def test_refused_options(lib):
    ok = lambda **kw: lib.photo_refine_ref_opts_valid(C.byref(_opts(**kw)))
    assert ok() and ok(levels=1) and ok(levels=4) and ok(sigma_floor_px=0.0) and ok(max_mse=3.0)
    d = _capi.PhotoRefineOpts()
    d.align = R.opts()
    d.levels, d.sigma_floor_px = 3, 0.05
    assert not lib.photo_refine_ref_opts_valid(C.byref(d))                     # cov_scale = 0, the default: the caller must choose it
    for kw in (dict(levels=0), dict(levels=5), dict(cov_scale=0.0), dict(cov_scale=-1.0), dict(cov_scale=float("nan")), dict(cov_scale=float("inf")),
               dict(sigma_floor_px=-0.1), dict(sigma_floor_px=float("nan")), dict(max_mse=-1.0), dict(max_mse=float("inf"))):
        assert not ok(**kw), kw
    bad = _opts()
    bad.align.huber_k = -1.0
    assert not lib.photo_refine_ref_opts_valid(C.byref(bad))


def _refined(lib, st, p, net, gate, max_nis, script, max_ratio, refine, align_rec, accepted):
    s = st.copy()
    iters = len(net)
    nn, sc = np.ascontiguousarray(net, dtype=np.float32), np.ascontiguousarray(script)
    ar = np.ascontiguousarray(align_rec, R.REC).reshape(1)
    rec, prec, rout = np.zeros(iters, ti.INNOV), np.zeros(1 + iters, tg.PHOTO), np.zeros(1, REFINE)
    calls, acalls, x0 = C.c_int(0), C.c_int(0), np.full(8, np.nan, np.float32)
    u = lib.photo_refine_ref_iterated(C.c_void_p(s.ctypes.data), C.byref(p), iters, C.c_void_p(nn.ctypes.data), int(gate), C.c_double(max_nis), C.c_void_p(sc.ctypes.data),
                                      C.c_double(max_ratio), 0, C.byref(refine) if refine is not None else None, C.c_void_p(ar.ctypes.data), int(accepted),
                                      C.c_void_p(rec.ctypes.data), C.c_void_p(prec.ctypes.data), C.c_void_p(rout.ctypes.data), C.byref(calls), C.byref(acalls),
                                      C.c_void_p(x0.ctypes.data))
    return s, u, rec, prec, rout[0], calls.value, acalls.value, x0


def _gated(lib, st, p, net, gate, max_nis, script, max_ratio):
    s = st.copy()
    iters = len(net)
    nn, sc = np.ascontiguousarray(net, dtype=np.float32), np.ascontiguousarray(script)
    rec, prec = np.zeros(iters, ti.INNOV), np.zeros(1 + iters, tg.PHOTO)
    calls = C.c_int(0)
    u = lib.photo_refine_ref_iterated_gated(C.c_void_p(s.ctypes.data), C.byref(p), iters, C.c_void_p(nn.ctypes.data), int(gate), C.c_double(max_nis),
                                            C.c_void_p(sc.ctypes.data), C.c_double(max_ratio), 0, C.c_void_p(rec.ctypes.data), C.c_void_p(prec.ctypes.data), C.byref(calls))
    return s, u, rec, prec, calls.value


def _setup(records, seed, iters=3):
    rng = np.random.default_rng(seed)
    p = ti._params()
    st = ti._state(rng)
    net = np.stack([ti._net(rng, st, 4.0) for _ in range(iters)])
    prior32 = (st["offset"][0][:, :2].reshape(8) * ti.F).astype(np.float32)
    rec, acc = records["spoiled"]
    rec = rec.copy()
    rec["px"]["offsets_px"] = prior32 + np.float32(0.3) * rng.standard_normal(8).astype(np.float32)      # an alignment that ended near this state's prior
    return p, st, net, prior32, rec, acc


def _same_as_gated(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()


@pytest.mark.parametrize("iters", [1, 3])
def test_no_fallback_is_iterated_update_photo_gated(lib, records, iters):
    """no refusal with refinement on; a refusal at iteration 0 with refinement off; a refusal at iteration 1; a closed reference gate: state, return value,
    innovation and photometric records are iterated_update_photo_gated's byte for byte, the aligner is never called and the refine record is zero"""
    p, st, net, _, rec, acc = _setup(records, 20 + iters, iters)
    o = _opts()
    cases = [("no refusal", [0.5] * iters, o, 1, 0.0), ("refinement off", [9.0] + [0.5] * (iters - 1), None, 1, 0.0), ("closed gate", [9.0] * iters, o, 0, 0.0),
             ("no refusal, NIS gate", [0.5] * iters, o, 1, 1e-3)]
    if iters > 1:
        cases.append(("refusal at 1", [0.5, 9.0] + [0.5] * (iters - 2), o, 1, 0.0))
    for name, ratios, refine, gate, max_nis in cases:
        sc = tg._script(ratios)
        want = _gated(lib, st, p, net, gate, max_nis, sc, 2.0)
        got = _refined(lib, st, p, net, gate, max_nis, sc, 2.0, refine, rec, acc)
        assert _same_as_gated(got, want), name
        assert got[5] == want[4] == iters and got[6] == 0 and got[4].tobytes() == np.zeros(1, REFINE).tobytes(), name


@pytest.mark.parametrize("iters", [1, 3])
def test_fallback_is_update_by_hand(lib, records, iters):
    """a refusal at iteration 0 with refinement on: the aligner is called once with iteration 0's fp32 prior; the state equals, byte for byte, update called
    by hand on the propagated state with refine_measurement's packed record and update_offset = 0, then reset_4pt_offset; the return value counts it;
    the refine record holds the aligner's record, R_px and hnet_ekf::innovation of the measurement; the other records are the refusal's"""
    p, st, net, prior32, rec, acc = _setup(records, 30 + iters, iters)
    o = _opts(cov_scale=3.0)
    sc = tg._script([9.0] + [0.5] * (iters - 1))
    refusal = _gated(lib, st, p, net, 1, 0.0, sc, 2.0)
    s, u, irec, prec, rout, calls, acalls, x0 = _refined(lib, st, p, net, 1, 0.0, sc, 2.0, o, rec, acc)
    assert acalls == 1 and calls == iters and x0.tobytes() == prior32.tobytes()
    ok, m72, r_px, fl = _measure(lib, rec, acc, o, p.k_net_cov)
    assert ok == 1 and fl == 0
    hand = st.copy()
    assert lib.photo_refine_ref_update(C.c_void_p(hand.ctypes.data), C.byref(p), C.c_void_p(m72.ctypes.data), 0, 1) == 1
    assert s.tobytes() == hand.tobytes() and s.tobytes() != refusal[0].tobytes()
    assert u == 1 and refusal[1] == 0
    assert irec.tobytes() == refusal[2].tobytes() and prec.tobytes() == refusal[3].tobytes() and list(irec["flag"]) == [tg.SKIPPED] * iters
    assert rout["flags"] == ASKED | APPLIED and rout["pad"] == 0
    assert rout["rec"].tobytes() == rec.tobytes() and rout["r_px"].tobytes() == r_px.tobytes()
    inn = np.zeros(1, ti.INNOV)
    assert lib.photo_refine_ref_innovation(C.c_void_p(st.ctypes.data), C.byref(p), C.c_void_p(m72.ctypes.data), C.c_void_p(inn.ctypes.data)) == 1
    inn["iteration"] = iters
    assert rout["innov"].tobytes() == inn[0].tobytes() and rout["innov"]["flag"] == tg.USED and np.isfinite(rout["innov"]["nis"])
    # the measurement pulls the state: the IMU block moved, the offsets are reset
    assert np.all(s["offset"] == 0) and np.all(s["cov"][0][15:, :] == 0) and s["p"].tobytes() != st["p"].tobytes()


def test_fallback_refused_or_unusable_leaves_the_refusal(lib, records):
    """a NIS gate that refuses the fallback, an unusable record and a singular S: the state is the one the refusal alone leaves"""
    p, st, net, _, rec, acc = _setup(records, 41, 3)
    o = _opts()
    sc = tg._script([9.0, 0.5, 0.5])
    refusal = _gated(lib, st, p, net, 1, 1e-12, sc, 2.0)
    s, u, irec, prec, rout, _, acalls, _ = _refined(lib, st, p, net, 1, 1e-12, sc, 2.0, o, rec, acc)
    assert acalls == 1 and u == 0 and s.tobytes() == refusal[0].tobytes() and irec.tobytes() == refusal[2].tobytes() and prec.tobytes() == refusal[3].tobytes()
    assert rout["flags"] == ASKED | NIS_REJECTED and rout["innov"]["flag"] == tg.REJECTED and rout["innov"]["nis"] > 1e-12 and rout["innov"]["iteration"] == 3
    assert rout["r_px"].any()
    # unusable: nothing accepted
    refusal = _gated(lib, st, p, net, 1, 0.0, sc, 2.0)
    s, u, _, _, rout, _, acalls, _ = _refined(lib, st, p, net, 1, 0.0, sc, 2.0, o, rec, 0)
    assert acalls == 1 and u == 0 and s.tobytes() == refusal[0].tobytes()
    assert rout["flags"] == ASKED | NO_STEP and rout["rec"].tobytes() == rec.tobytes() and not rout["r_px"].any()
    assert rout["innov"]["flag"] == tg.NONE and rout["innov"]["iteration"] == 3 and not rout["innov"]["r"].any() and rout["innov"]["nis"] == 0.0
    # singular S: a zero state covariance and a zero R_px (mse = 0, no floor)
    zs = st.copy()
    zs["cov"] = 0.0
    zrec = rec.copy()
    zrec["px"]["mse"] = 0.0
    refusal = _gated(lib, zs, p, net, 1, 0.0, sc, 2.0)
    s, u, _, _, rout, _, _, _ = _refined(lib, zs, p, net, 1, 0.0, sc, 2.0, _opts(sigma_floor_px=0.0), zrec, acc)
    assert u == -1 and s.tobytes() == refusal[0].tobytes() and rout["flags"] == ASKED | S_SINGULAR and rout["innov"]["flag"] == tg.SINGULAR and np.isnan(rout["innov"]["nis"])


def test_photo_refine_header_under_asan_ubsan(tmp_path):
    """the header on a synthetic record and a scripted loop under AddressSanitizer + UBSan: a stand-alone program; nothing loaded into python is sanitized"""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    exe = str(tmp_path / "filters_photo_refine_check_san.bin")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *san, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filters_photo_refine_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "photo refine check: measurement, 8 unusable cases, 5 loop paths (1 applied) ok" in r.stdout, r.stdout
