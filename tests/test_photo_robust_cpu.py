"""Photometric alignment with a gain / bias model and Huber weights (include/hnet.h hnet_op_photo_align_robust; include/hnet_photo_robust.h)
on the CPU: the host reference tests/cpp/photo_robust_ref.cpp - the quantity, the reduction, the step and the level loop on the functions the device
compiles - against the coarse-to-fine reference (model off, k = 0: byte for byte), central differences of its float64 twin in all ten parameters, the
truth of pairs with an exposure step and a foreign block, the hostile starts, hnet_photo_robust_marginal against numpy, and its core under
AddressSanitizer + UBSan (tests/cpp/photo_robust_check.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import photo_align_pyr_util as P
import photo_align_util as U
import photo_robust_util as R
from cuahn_vio_amd import _capi
from cuahn_vio_amd.weights import uniform01

ROOT = U.ROOT
# measured worst over the cases of test_gradient_is_the_derivative_of_the_robust_cost (relative to the largest offset component, |g gain|, |g bias|):
# central differences against the twin's gradient 3.0e-8; the fp32 quantity's gradient against the twin's 2.5e-5.  Gates: 10 x
MEASURED_FD, MEASURED_G32 = 3.0e-8, 2.5e-5


@pytest.fixture(scope="module")
def rref(tmp_path_factory):
    return R.build_ref(tmp_path_factory.mktemp("photo_robust_ref"))


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return P.build_ref(tmp_path_factory.mktemp("photo_align_pyr_ref_for_robust"))


def _model_off_fields(r):
    x = r["px"]
    assert r["gain"] == 1.0 and r["bias"] == 0.0 and r["n_outliers0"] == 0 and r["n_outliers"] == 0
    assert not r["info10"][8:].any() and not r["info10"][:, 8:].any() and not r["grad10"][8:].any()
    assert r["info10"][:8, :8].tobytes() == np.ascontiguousarray(x["info"]).tobytes() and r["grad10"][:8].tobytes() == x["grad"].tobytes()


def test_model_off_is_the_pyramid_reference_at_one_level(rref, pref):
    """brightness = 0, huber_k = 0, levels = 1: the common part of every record equals photo_align_pyr_ref_run byte for byte on the 12 convergence cases,
    at 6 trials and at none; gain / bias stay 1 / 0, rows and columns 8, 9 of info10 are zero and its 8 x 8 block is px.info"""
    cs = U.convergence_cases()
    i1, i2, start = np.stack([c[1] for c in cs]), np.stack([c[2] for c in cs]), np.stack([c[4] for c in cs])
    for K in (6, 0):
        want, _ = P.ref_run(pref, i1, i2, start, 1, max_iterations=K)
        out, lv = R.ref_run(rref, i1, i2, start, 1, max_iterations=K, brightness=0, huber_k=0.0)
        for i, c in enumerate(cs):
            assert out[i]["px"].tobytes() == want[i].tobytes(), (c[0], K)
            assert out[i].tobytes() == lv[i, 0].tobytes()
            _model_off_fields(out[i])


def test_model_off_is_the_pyramid_reference_at_four_levels(rref, pref):
    """the same at levels = 4 with 8 trials per level on the four basin pairs (max_offset 32), every level's record"""
    i1, i2, _ = P.basin_cases(32.0)
    _, want = P.ref_run(pref, i1, i2, np.zeros((4, 8), np.float32), 4, max_iterations=8)
    _, lv = R.ref_run(rref, i1, i2, np.zeros((4, 8), np.float32), 4, max_iterations=8, brightness=0, huber_k=0.0)
    for i in range(4):
        for L in range(4):
            assert lv[i, L]["px"].tobytes() == want[i, L].tobytes(), (i, L)
            _model_off_fields(lv[i, L])


STEP = np.array([1e-3] * 8 + [1e-5, 1e-3])


@pytest.mark.parametrize("level,k", [(0, 0.0), (1, 0.0), (2, 10.0), (3, 10.0)])
@pytest.mark.parametrize("kind,seed", [("smooth", 1), ("stock", 2), ("smooth", 5), ("stock", 11)])
def test_gradient_is_the_derivative_of_the_robust_cost(rref, kind, seed, level, k):
    """g10 equals the central differences of sum rho / 2 in each of the ten parameters (steps 1e-3 px, 1e-5 of gain, 1e-3 grey levels) on the float64
    twin, on a pair with the exposure step, at gain 1.3 and bias -30 (away from the optimum: no component of g is small) and offsets where no sample
    crosses a cell border; the valid and the outlier counts are equal at p and p +- step, so no |r| crosses k within the step (k = 10 at levels 2 and 3,
    where that holds on all four pairs; at levels 0 and 1 some pixel of 70 000 always does).  Each component is held relative to its block: the largest
    offset component, |g gain|, |g bias|.  The fp32 quantity's g10 agrees with the twin's within 10 x MEASURED_G32."""
    i1, i2 = (U.smooth_pair(seed, 2.0) if kind == "smooth" else U.stock_pair(seed))[:2]
    i2 = R.spoil(i2)
    x = (0.5 + (uniform01(seed, 4004, 8).astype(np.float64) * 2.0 - 1.0) * 0.3) * (1 << level)
    p = np.concatenate([x, [1.3, -30.0]])
    _, g, n, n_out, margin = R.ref_cost64(rref, i1, i2, p, k, level)
    fd = np.zeros(10)
    for j in range(10):
        e = np.zeros(10)
        e[j] = STEP[j]
        cp, _, n_p, o_p, _ = R.ref_cost64(rref, i1, i2, p + e, k, level)
        cm, _, n_m, o_m, _ = R.ref_cost64(rref, i1, i2, p - e, k, level)
        assert n_p == n_m == n == (P.LEVEL_W[level] - 1) * (P.LEVEL_H[level] - 1) and o_p == o_m == n_out
        fd[j] = (cp - cm) / (2.0 * STEP[j])
    scale = np.array([np.abs(g[:8]).max()] * 8 + [abs(g[8]), abs(g[9])])
    rel = float((np.abs(fd - g) / scale).max())
    sums, ok = R.ref_sums(rref, i1, i2, x.astype(np.float32), p[8], p[9], k, level)
    _, g32 = R.ref_reduce(rref, x.astype(np.float32), p[8], sums)
    rel32 = float((np.abs(g32[0] - g) / scale).max())
    print(f"level {level} {kind} {seed} k {k}: |fd - g| / scale = {rel:.2e}; fp32 quantity vs float64 twin {rel32:.2e}; outliers {n_out} of {n}, "
          f"nearest |r| to k {margin:.1e}")
    assert ok[0] == 1 and sums["n_valid"][0] == n and (k == 0.0) == (n_out == 0) and (k == 0.0 or margin > 0.0)
    assert rel < 10 * MEASURED_FD
    assert rel32 < 10 * MEASURED_G32


def test_marginal_is_the_schur_complement(rref):
    """hnet_photo_robust_marginal equals the inverse of the top-left 8 x 8 of inverse(info10), and its gradient g_x - A_xc A_cc^-1 g_c, to 1e-9 relative,
    on the records of an accuracy row; with the model off it copies px.info / px.grad; a brightness block without a Cholesky factor is refused and
    nothing is written"""
    i1, i2, _, start = R.row_pairs("block-1level")
    out, _ = R.ref_run(rref, i1, i2, start, 1, max_iterations=4, huber_k=10.0)
    for r in out:
        info, grad = _capi.photo_robust_marginal(r)
        A, g = r["info10"].astype(np.float64), r["grad10"].astype(np.float64)
        want = np.linalg.inv(np.linalg.inv(A)[:8, :8])
        want_g = g[:8] - A[:8, 8:] @ np.linalg.solve(A[8:, 8:], g[8:])
        assert np.abs(info - want).max() <= 1e-9 * np.abs(want).max()
        assert np.abs(grad - want_g).max() <= 1e-9 * np.abs(want_g).max()
        assert (info == info.T).all()
    off, _ = R.ref_run(rref, i1[:1], i2[:1], start[:1], 1, max_iterations=2, brightness=0, huber_k=0.0)
    info, grad = _capi.photo_robust_marginal(off[0])
    assert info.tobytes() == np.ascontiguousarray(off[0]["px"]["info"]).tobytes() and grad.tobytes() == off[0]["px"]["grad"].tobytes()
    bad = out[:1].copy()
    bad["info10"][0, 9, 9] = bad["info10"][0, 8, 9] ** 2 / bad["info10"][0, 8, 8] * (1 - 1e-3)        # a negative second pivot
    info, grad = np.full((8, 8), 7.0), np.full(8, 7.0)
    rc = _capi.lib().hnet_photo_robust_marginal(C.c_void_p(bad.ctypes.data), C.c_void_p(info.ctypes.data), C.c_void_p(grad.ctypes.data))
    assert rc != 0 and (info == 7.0).all() and (grad == 7.0).all()


@pytest.mark.parametrize("name", list(R.ROWS))
def test_accuracy_rows(rref, pref, name):
    """an exposure step of gain 0.7 / bias +25 (and, in the block rows, 40 x 60 pixels of noise with k = 10) on seeds 1, 2, 5, 11: the reference ends
    within the row's gate of the truth (twice its own worst, R.ROWS), and the coarse-to-fine reference without the model, on the same pair from the same
    start with the same trials, ends at least 3 x further away (except R.RATIO_DROPPED, which never kept that ratio).  Measured (worst component, px):
      gain-1level    0.016 0.025 0.041 0.006 against 0.116 0.441 0.147 0.673     gain-4levels   0.008 0.006 0.018 0.009 against 0.082 0.103 0.173 0.188
      block-1level   0.073 0.039 0.050 0.025 against 0.371 0.092 0.247 0.143     block-4levels  0.025 0.046 0.050 0.022 against 0.237 0.260 0.176 0.252"""
    levels, kw = R.row_opts(name)
    gate = R.ROWS[name][4]
    i1, i2, truth, start = R.row_pairs(name)
    out, lv = R.ref_run(rref, i1, i2, start, levels, **kw)
    old, _ = P.ref_run(pref, i1, i2, start, levels, max_iterations=kw["max_iterations"])
    for i, seed in enumerate(U.SEEDS):
        err = R.worst_px(out[i], truth[i])
        err_old = float(np.abs(old[i]["offsets_px"].astype(np.float64) - truth[i]).max())
        report = (f"{name} seed {seed}: {err:.4f} px off (gate {gate:.4f}), without the model {err_old:.4f} px ({err_old / err:.1f} x), gain {out[i]['gain']:.4f}, "
                  f"bias {out[i]['bias']:.3f}\n{R.describe_levels(lv[i], truth[i])}")
        print(report)
        assert err < gate, report
        if (name, seed) not in R.RATIO_DROPPED:
            assert err_old >= R.RATIO * err, report
        # the model is applied to img2, which was made from img1's scene by x 0.7 + 25: the gain found is near 1 / 0.7 and the bias near -25 / 0.7
        assert 1.35 < out[i]["gain"] < 1.5 and -42.0 < out[i]["bias"] < -33.0, report
        assert (out[i]["n_outliers"] > 1500) == R.ROWS[name][2], report


def _finite(r):
    x = r["px"]
    return all(np.isfinite(v).all() for v in (x["mse0"], x["mse"], x["lambda"], x["grad"], x["info"], r["gain"], r["bias"], r["grad10"], r["info10"]))


@pytest.mark.parametrize("i", range(len(R.hostile_cases())), ids=[c[0] for c in R.hostile_cases()])
def test_hostile_starts_at_four_levels(rref, i):
    """with the model on and k = 10, at four levels: a constant img2 is SINGULAR at every level with the offsets, gain and bias bit for bit and info10
    zero outside the brightness block; stripes SINGULAR; the collinear and NaN starts DEGENERATE, the far start FEW_PIXELS, with a zero info10;
    gain0 = 1e-30 and 1e30 and k = 1e-6 (every pixel with r != 0 an outlier) leave finite records with a positive gain"""
    name, i1, i2, start, kw, flag = R.hostile_cases()[i]
    for K in (8, 0):
        out, lv = R.ref_run(rref, i1, i2, start, 4, max_iterations=K, **kw)
        print(f"{name}, K = {K}:\n{R.describe_levels(lv[0])}")
        assert out[0].tobytes() == lv[0, 0].tobytes()
        for L in range(4):
            r, x = lv[0, L], lv[0, L]["px"]
            assert x["accepted"] <= x["trials"] <= K and r["gain"] > 0 and 0 <= r["n_outliers"] <= x["n_valid"] and r["n_outliers0"] <= x["n_valid0"]
            if name != "nan":
                assert _finite(r), (name, L)
            if flag is not None:
                assert x["flags"] == flag and x["trials"] == 0 and x["offsets_px"].tobytes() == start.tobytes() and r["gain"] == 1.0 and r["bias"] == 0.0
            if flag in (U.DEGENERATE, U.FEW_PIXELS):
                assert x["n_valid0"] == 0 and x["mse0"] == 0.0 and not r["info10"].any() and not r["grad10"].any() and r["n_outliers0"] == 0
            if name == "constant":
                assert not r["info10"][:8].any() and not x["info"].any() and r["info10"][9, 9] > 0
            if name == "all-outliers":
                assert r["n_outliers0"] > 0.9 * x["n_valid0"] and x["mse"] <= x["mse0"]
    if name == "nan":
        assert out[0]["px"]["offsets_px"].view(np.uint32)[3] == 0x7FC12345


def test_a_flat_frame_with_one_textured_stripe(rref):
    """img2 flat but for eight textured rows: the few pixels with a gradient carry the offsets, all of them carry gain and bias; the record stays finite
    at every level and the cost does not rise"""
    i1, i2, _ = U.smooth_pair(1, 2.0)
    flat = np.full((224, 320), 93, np.uint8)
    flat[100:108] = i2[100:108]
    for K in (8, 0):
        _, lv = R.ref_run(rref, i1, flat, np.zeros(8, np.float32), 4, max_iterations=K)
        print(R.describe_levels(lv[0]))
        for L in range(4):
            assert _finite(lv[0, L]) and lv[0, L]["px"]["mse"] <= lv[0, L]["px"]["mse0"] and lv[0, L]["gain"] > 0
            assert not lv[0, L]["px"]["flags"] & (U.DEGENERATE | U.FEW_PIXELS)


def test_a_trial_with_a_negative_gain_is_refused(rref):
    """img2 = 255 - img2 of a smooth pair: the least-squares gain is negative.  The first step, recomputed here from info10 / grad10 of the start record,
    takes the gain below zero to a point whose mean cost IS smaller (the reference's sums at that point say so): only the rule on the gain refuses it.
    The trial is counted, not accepted, lambda grows, and whatever follows keeps the gain positive."""
    i1, i2, _ = U.smooth_pair(1, 2.0)
    neg = (255 - i2.astype(np.int32)).astype(np.uint8)
    zero = np.zeros(8, np.float32)
    r0, _ = R.ref_run(rref, i1, neg, zero, 1, max_iterations=0, huber_k=0.0)
    A, g, lam = r0[0]["info10"].astype(np.float64), r0[0]["grad10"].astype(np.float64), float(r0[0]["px"]["lambda"])
    dp = -np.linalg.solve(A + lam * np.diag(np.diag(A)), g)
    assert 1.0 + dp[8] < 0.0
    sums, _ = R.ref_sums(rref, i1, neg, (zero + dp[:8]).astype(np.float32), 1.0 + dp[8], dp[9], 0.0, 0)
    assert sums["rho"][0] / sums["n_valid"][0] < r0[0]["px"]["mse0"] and sums["n_valid"][0] >= 20000
    r1, _ = R.ref_run(rref, i1, neg, zero, 1, max_iterations=1, huber_k=0.0)
    x = r1[0]["px"]
    assert x["trials"] == 1 and x["accepted"] == 0 and x["lambda"] == lam * 10.0 and r1[0]["gain"] == 1.0 and x["mse"] == x["mse0"]
    r8, _ = R.ref_run(rref, i1, neg, zero, 1, max_iterations=8, huber_k=0.0)
    print(R.describe_levels(r8))
    assert r8[0]["px"]["trials"] > r8[0]["px"]["accepted"] and r8[0]["gain"] > 0.0 and _finite(r8[0])


def test_refused_options(rref):
    """hnet_robust::opts_valid, what the C API answers HNET_ERR_INVALID_ARG by: the base options' rules, brightness outside 0 / 1, a negative or
    non-finite huber_k, a non-finite or non-positive gain0, a non-finite bias0, and a start other than 1 / 0 with the model off"""
    ok = lambda **kw: rref.photo_robust_ref_opts_valid(C.byref(R.opts(**kw)))
    assert ok() and ok(brightness=0, huber_k=0.0) and ok(gain0=1e-30) and ok(gain0=1e30, bias0=-300.0) and ok(huber_k=0.0)
    for kw in (dict(brightness=2), dict(brightness=-1), dict(huber_k=-1.0), dict(huber_k=float("nan")), dict(huber_k=float("inf")), dict(gain0=0.0),
               dict(gain0=-1.0), dict(gain0=float("nan")), dict(gain0=float("inf")), dict(bias0=float("nan")), dict(bias0=float("inf")),
               dict(brightness=0, gain0=1.1), dict(brightness=0, bias0=1.0), dict(max_iterations=33), dict(lambda0=0.0), dict(min_valid=-1)):
        assert not ok(**kw), kw


def test_photo_robust_check_under_asan_ubsan(tmp_path):
    """the reference core on its fixed scene with an exposure step and a foreign block, the model-off identity and the hostile starts under
    AddressSanitizer + UBSan: a stand-alone program; nothing loaded into python is sanitized"""
    exe = str(tmp_path / "photo_robust_check_san.bin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *U.HOST_FLAGS,
                    os.path.join(ROOT, "tests", "cpp", "photo_robust_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "photo_robust_check: ok" in r.stdout
