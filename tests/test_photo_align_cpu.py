"""Photometric alignment (include/hnet.h hnet_photo_align; include/hnet_photo_align.h) on the CPU: the host reference
tests/cpp/photo_align_ref.cpp - the quantity restated on photo_ref.cpp's fp32 sampler, reduced and stepped by the functions the device compiles - against
central differences, the truth of synthetic pairs and the degenerate inputs, and its core under AddressSanitizer + UBSan (tests/cpp/photo_align_check.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import photo_align_util as U
from cuahn_vio_amd.weights import uniform01

ROOT = U.ROOT
P4 = np.array([0, 0, 0, 223, 319, 223, 319, 0], np.float64)


@pytest.fixture(scope="module")
def aref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp("photo_align_ref"))


@pytest.fixture(scope="module")
def converged(aref):
    """the host reference on every convergence case at K = 10 and K = 6, once for the module: {(name, K): record}"""
    cases = U.convergence_cases()
    i1, i2 = np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])
    start = np.stack([c[4] for c in cases])
    return {K: U.ref_run(aref, i1, i2, start, max_iterations=K) for K in (6, 10)}


def _kink_free_point(seed):
    """offsets 0.5 +- 0.3 px per component: every pixel samples within 0.2 .. 0.8 of a cell of img2 (the position of a pixel lies between those of
    the corners up to the perspective term, < 1e-3 px here), so that a move of 1e-3 px takes no sample across a cell border, where the bilinear
    interpolant has a kink and central differences of the cost say nothing about its derivative; and n_valid is the same at x +- step."""
    return 0.5 + (uniform01(seed, 4004, 8).astype(np.float64) * 2.0 - 1.0) * 0.3


@pytest.mark.parametrize("kind", ["smooth", "stock"])
@pytest.mark.parametrize("seed", U.SEEDS)
def test_gradient_is_the_derivative_of_the_cost(aref, seed, kind):
    """1. g equals the central differences of sum r^2 / 2 in each of the 8 offsets, step 1e-3 px, at 1e-5 of max |g|, on points where n_valid is equal at
    x +- step.  The differences are taken on the float64 twin of the quantity (photo_align_ref_cost64): the fp32 sampler's positions carry a rounding
    of up to a few ulp of 319 (3e-5 px), 3 % of the step.  Measured: 5.3e-8 at worst over the 8 pairs.
    The fp32 quantity's g is then held against the twin's: the same 3e-5 px in the positions moves a residual by |gradient| * 3e-5; measured
    3.5e-5 of max |g| at worst over the 8 pairs, gated at 10 x that, so that an error in the fp32 row s cannot hide under the gate."""
    i1, i2 = (U.smooth_pair(seed, 2.0) if kind == "smooth" else U.stock_pair(seed))[:2]
    x = _kink_free_point(seed)
    _, g, n = U.ref_cost64(aref, i1, i2, x)
    fd = np.zeros(8)
    for k in range(8):
        e = np.zeros(8)
        e[k] = 1e-3
        cp, _, n_p = U.ref_cost64(aref, i1, i2, x + e)
        cm, _, n_m = U.ref_cost64(aref, i1, i2, x - e)
        assert n_p == n_m == n == 223 * 319
        fd[k] = (cp - cm) / 2e-3
    rel = np.abs(fd - g).max() / np.abs(g).max()
    sums, ok = U.ref_sums(aref, i1, i2, x.astype(np.float32))
    _, g32 = U.ref_reduce(aref, x.astype(np.float32), sums)
    rel32 = np.abs(g32[0] - g).max() / np.abs(g).max()
    print(f"{kind} {seed}: |fd - g| / max |g| = {rel:.2e}; fp32 quantity vs float64 twin {rel32:.2e}")
    assert ok[0] == 1 and sums["n_valid"][0] == n
    assert rel < 1e-5
    assert rel32 < 3.5e-4


def test_dlt_jacobian_is_the_derivative_of_dlt_solve(aref):
    """2. D = dvec(H) / dx against central differences of csrc/geom.h's dlt_solve (step 1e-3 px), per row of D relative to the row's largest entry, on
    quadrilaterals up to 40 px from the rectangle.  Measured worst: 6.3e-11 (the differences' own rounding: 1e-16 * |H| / 1e-3 on the rows of h13, h23;
    the truncation term vanishes to second order); gated at 10 x that.  Row 9 (h33 = 1) is exactly zero."""
    worst = 0.0
    for seed in U.SEEDS:
        for mo in (0.0, 2.0, 12.0, 40.0):
            dst = P4 + (uniform01(seed, 5005, 8).astype(np.float64) * 2.0 - 1.0) * mo
            H, D = np.zeros(9), np.zeros((9, 8))
            aref.photo_align_ref_dlt(C.c_void_p(dst.ctypes.data), C.c_void_p(H.ctypes.data), C.c_void_p(D.ctypes.data))
            fd = np.zeros((9, 8))
            for k in range(8):
                for sgn in (1.0, -1.0):
                    d2, H2, D2 = dst.copy(), np.zeros(9), np.zeros((9, 8))
                    d2[k] += sgn * 1e-3
                    aref.photo_align_ref_dlt(C.c_void_p(d2.ctypes.data), C.c_void_p(H2.ctypes.data), C.c_void_p(D2.ctypes.data))
                    fd[:, k] += sgn * H2 / 2e-3
            assert not D[8].any() and not fd[8].any()
            worst = max(worst, float((np.abs(fd - D)[:8].max(axis=1) / np.abs(D)[:8].max(axis=1)).max()))
    print(f"worst row-relative |fd - D| = {worst:.2e}")
    assert worst < 6.3e-10


@pytest.mark.parametrize("i", range(12), ids=[c[0] for c in U.convergence_cases()])
def test_converges_to_the_truth(converged, i):
    """3. K = 10, and the default K = 6: smooth pairs (max_offset 2 and 8) from zero offsets end within 0.05 px of the true offsets in every component, stock pairs
    (max_offset 12) from the sigma = 1 prior within 0.1 px; seeds 1, 2, 5, 11.  Measured with this reference: smooth <= 0.019 px at max_offset 2,
    <= 0.0063 px at 8, stock <= 0.039 px from starts 1.4 - 1.7 px off.
    The same worst figures hold at K = 6.
    4. mse <= mse0, accepted <= trials <= K."""
    name, _i1, _i2, truth, start, gate = U.convergence_cases()[i]
    for K in (10, 6):
        r = converged[K][i]
        err = float(np.abs(r["offsets_px"].astype(np.float64) - truth).max())
        print(f"{name} K={K}: start {np.abs(start - truth).max():.3f} px off, end {err:.4f} px off; mse {r['mse0']:.3f} -> {r['mse']:.3f}; "
              f"trials {r['trials']}, accepted {r['accepted']}, flags {r['flags']}")
        assert r["mse"] <= r["mse0"] and 0 <= r["accepted"] <= r["trials"] <= K
        assert r["flags"] in (0, U.CONVERGED)
        assert np.isfinite(r["info"]).all() and (r["info"] == r["info"].T).all()
        assert err < gate


def test_linearisation_alone(aref):
    """K = 0: the start offsets come back with info, grad, mse at them and no trial; on the identity hypothesis n_valid = 223 * 319"""
    i1, i2, _ = U.smooth_pair(1, 2.0)
    r = U.ref_run(aref, i1, i2, np.zeros(8), max_iterations=0)[0]
    assert r["trials"] == 0 and r["accepted"] == 0 and r["flags"] == 0 and r["mse"] == r["mse0"] > 0
    assert r["n_valid0"] == r["n_valid"] == 223 * 319 and not r["offsets_px"].any()
    sums, _ = U.ref_sums(aref, i1, i2, np.zeros(8))
    A, g = U.ref_reduce(aref, np.zeros(8), sums)
    assert (r["info"] == A[0]).all() and (r["grad"] == g[0]).all() and r["mse"] == sums["rr"][0] / sums["n_valid"][0]
    assert np.linalg.eigvalsh(A[0]).min() > 0


@pytest.mark.parametrize("i", range(4), ids=[c[0] for c in U.degenerate_cases()])
def test_degenerate_inputs(aref, i):
    """5. a constant img2: info exactly zero, SINGULAR, the start offsets bit for bit; identical rows (vertical stripes): SINGULAR; a start without a
    homography: DEGENERATE; a start 400 px off: FEW_PIXELS; no non-finite output in any of them, with K = 0 as with K = 6.
    On the stripes A is NOT zero in its v rows - moving a corner in v changes the perspective terms h31, h32 and with them every ix - but the image
    depends on ix alone, which has 5 parameters: A has rank 5 (its three smallest eigenvalues measure 1e-16 of the largest and less) and its sixth
    Cholesky pivot is rounding noise, far below the rule's 1e-12 of max diag(A)."""
    name, i1, i2, start, flag, zero = U.degenerate_cases()[i]
    for K in (0, 6):
        r = U.ref_run(aref, i1, i2, start, max_iterations=K)[0]
        assert r["flags"] == flag, name
        assert r["offsets_px"].tobytes() == start.tobytes() and r["trials"] == 0 and r["accepted"] == 0
        for f in ("mse0", "mse", "lambda", "grad", "info"):
            assert np.isfinite(r[f]).all(), (name, f)
        if zero:
            assert not r["info"].any() and not r["grad"].any()
        if flag in (U.DEGENERATE, U.FEW_PIXELS):
            assert r["n_valid0"] == 0 and r["mse0"] == 0.0
        else:
            assert r["n_valid0"] == 223 * 319 and r["mse0"] > 0
    if name == "stripes":
        w = np.linalg.eigvalsh(r["info"])
        print(f"stripes: eigenvalues of A / largest: {w / w.max()}")
        assert (np.abs(w[:3]) < 1e-9 * w.max()).all() and w[3] > 1e-9 * w.max()


def test_photo_align_check_under_asan_ubsan(tmp_path):
    """6. the reference core and the step function on two fixed pairs under AddressSanitizer + UBSan (a stand-alone program)"""
    exe = str(tmp_path / "photo_align_check_san.bin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *U.HOST_FLAGS,
                    os.path.join(ROOT, "tests", "cpp", "photo_align_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "photo_align_check: ok" in r.stdout
