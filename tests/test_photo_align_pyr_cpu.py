"""Coarse-to-fine photometric alignment (include/hnet.h hnet_op_photo_align_pyramid; include/hnet_photo_pyramid.h) on the CPU: the host
reference tests/cpp/photo_align_pyr_ref.cpp - the pyramid, the per-level quantity and the loop over levels on the functions the device compiles -
against a numpy restatement of the pyramid, the single-level reference, the truth of pairs up to 32 px apart, the hostile starts, central differences
per level, and its core under AddressSanitizer + UBSan (tests/cpp/photo_align_pyr_check.cpp)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import photo_align_pyr_util as P
import photo_align_util as U
from cuahn_vio_amd import synth
from cuahn_vio_amd.weights import uniform01

ROOT = U.ROOT
BASIN_GATE_PX = 0.1             # the stock gate of tests/test_photo_align_cpu.py


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return P.build_ref(tmp_path_factory.mktemp("photo_align_pyr_ref"))


@pytest.fixture(scope="module")
def aref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp("photo_align_ref_for_pyr"))


def test_pyramid_is_the_rounded_box_mean(pref):
    """levels 1 .. 3 equal the numpy restatement (a + b + c + d + 2) >> 2, cascaded, bit for bit: a stock frame, a 0 / 255 checker (128 at every level)
    and an all-255 frame, which stays 255: the rounding term must not overflow a byte"""
    stock = synth.make_pair(1, 32.0)[0]
    vs, us = np.meshgrid(np.arange(224), np.arange(320), indexing="ij")
    checker = (((us + vs) & 1) * 255).astype(np.uint8)
    white = np.full((224, 320), 255, np.uint8)
    got = P.ref_pyramid(pref, np.stack([stock, checker, white]))
    for b, img in enumerate((stock, checker, white)):
        for want, have in zip(P.numpy_pyramid(img), P.split_pyramid(got[b])):
            assert want.shape == have.shape and (want == have).all()
    assert (got[1] == 128).all() and (got[2] == 255).all()
    assert len(np.unique(got[0])) > 100


def test_one_level_is_the_single_level_reference(pref, aref):
    """levels = 1 equals photo_align_ref_run byte for byte on the 12 convergence cases: level 0 of the per-level quantity is today's quantity"""
    cs = U.convergence_cases()
    i1, i2, start = np.stack([c[1] for c in cs]), np.stack([c[2] for c in cs]), np.stack([c[4] for c in cs])
    for K in (6, 0):
        want = U.ref_run(aref, i1, i2, start, max_iterations=K)
        out, lv = P.ref_run(pref, i1, i2, start, 1, max_iterations=K)
        for i, c in enumerate(cs):
            assert out[i].tobytes() == want[i].tobytes() == lv[i, 0].tobytes(), (c[0], K)
    sums0, ok0 = P.ref_sums(pref, i1[:3], i2[:3], start[:3], 0)
    sums, ok = U.ref_sums(aref, i1[:3], i2[:3], start[:3])
    assert sums0.tobytes() == sums.tobytes() and (ok0 == ok).all()


def _errors(lv, truth):
    return [float(np.abs(lv[L]["offsets_px"].astype(np.float64) - truth).max()) for L in range(len(lv))]


@pytest.mark.parametrize("max_offset", [32.0, 12.0])
def test_four_levels_reach_the_truth_from_zero(pref, max_offset):
    """synth.make_pair(seed, 32.0) and (seed, 12.0), seeds 1, 2, 5, 11, from zero offsets: levels = 4 with max_iterations = 8 per level ends within
    0.1 px of the truth in every component.  Measured with this reference: at most 0.018 px at 32, at most 0.041 px at 12."""
    i1, i2, truth = P.basin_cases(max_offset)
    out, lv = P.ref_run(pref, i1, i2, np.zeros((4, 8), np.float32), 4, max_iterations=8)
    for i, seed in enumerate(U.SEEDS):
        err = _errors(lv[i], truth[i])
        report = f"seed {seed}, max_offset {max_offset}: per-level error {['%.4f' % e for e in err]} px (index = level)\n{P.describe_levels(lv[i], truth[i])}"
        print(report)
        assert out[i].tobytes() == lv[i, 0].tobytes()
        assert err[0] < BASIN_GATE_PX, report
        for L in range(4):
            assert lv[i, L]["mse"] <= lv[i, L]["mse0"] and lv[i, L]["accepted"] <= lv[i, L]["trials"] <= 8, report
            assert not lv[i, L]["flags"] & (U.SINGULAR | U.DEGENERATE | U.FEW_PIXELS), report


def test_one_level_does_not_reach_it(pref):
    """the same four pairs at max_offset 32 with levels = 1 and max_iterations = 32 (the same 32 trials): more than 5 px off on every pair (measured:
    at least 13.3 px): the pyramid is what closes the distance, not the trial count"""
    i1, i2, truth = P.basin_cases(32.0)
    out, _ = P.ref_run(pref, i1, i2, np.zeros((4, 8), np.float32), 1, max_iterations=32)
    for i, seed in enumerate(U.SEEDS):
        err = float(np.abs(out[i]["offsets_px"].astype(np.float64) - truth[i]).max())
        print(f"seed {seed}: one level, 32 trials: {err:.2f} px off")
        assert err > 5.0, seed


@pytest.mark.parametrize("i", range(5), ids=[c[0] for c in P.hostile_cases()])
def test_hostile_starts_at_four_levels(pref, i):
    """on smooth_pair(1, 2.0): a constant img2 is SINGULAR at all four levels with info == 0 and the offsets bit for bit; stripes SINGULAR at all levels;
    the far start FEW_PIXELS at all levels with n_valid0 == 0; the collinear start DEGENERATE at all levels; a NaN start comes back with its payload.
    A level's flags stop that level only, and the next starts where it ended: here, where it started."""
    name, i1, i2, start, flag = P.hostile_cases()[i]
    for K in (8, 0):
        out, lv = P.ref_run(pref, i1, i2, start, 4, max_iterations=K)
        assert out[0].tobytes() == lv[0, 0].tobytes()
        for L in range(4):
            r = lv[0, L]
            assert r["flags"] == flag, (name, L, P.describe_levels(lv[0]))
            assert r["offsets_px"].tobytes() == start.tobytes() and r["trials"] == 0 and r["accepted"] == 0
            for f in ("mse0", "mse", "lambda", "grad", "info"):
                assert np.isfinite(r[f]).all(), (name, L, f)
            if name == "constant":
                # (at zero offsets a coarse level loses its first row and column too: the centre 2^L u + c of u = 0 comes back from the fp32
                # normalise / un-normalise round trip a few ulp below c, so ix < 0)
                assert not r["info"].any() and not r["grad"].any() and r["n_valid0"] == (P.LEVEL_W[L] - 1 - (L > 0)) * (P.LEVEL_H[L] - 1 - (L > 0))
            if flag in (U.DEGENERATE, U.FEW_PIXELS):
                assert r["n_valid0"] == 0 and r["mse0"] == 0.0 and not r["info"].any()
    if name == "nan":
        assert out[0]["offsets_px"].view(np.uint32)[3] == 0x7FC12345


def test_min_valid_scales_with_the_level(pref):
    """min_valid = 20000 asks 20000 >> 6 = 312 pixels of level 3.  A shift of 224 px leaves level 3 eleven columns of 26 rows, 286 pixels (chosen on this
    reference): FEW_PIXELS there at the default, not at min_valid = 64 * 286, where level 3 needs exactly its own count"""
    i1, i2, _ = U.smooth_pair(1, 2.0)
    start = np.tile(np.array([224.0, 0.0], np.float32), 4)
    _, free = P.ref_run(pref, i1, i2, start, 4, max_iterations=0, min_valid=0)
    n3 = int(free[0, 3]["n_valid0"])
    print(f"level 3 at a shift of 224 px: {n3} valid pixels; levels 2, 1, 0: {[int(free[0, L]['n_valid0']) for L in (2, 1, 0)]}")
    assert 9 <= n3 <= 311 and not free[0, 3]["flags"] & U.FEW_PIXELS
    _, lv = P.ref_run(pref, i1, i2, start, 4, max_iterations=0, min_valid=20000)
    assert lv[0, 3]["flags"] == U.FEW_PIXELS and lv[0, 3]["n_valid0"] == n3 and lv[0, 3]["offsets_px"].tobytes() == start.tobytes()
    _, lv = P.ref_run(pref, i1, i2, start, 4, max_iterations=0, min_valid=64 * n3)
    assert not lv[0, 3]["flags"] & U.FEW_PIXELS
    _, lv = P.ref_run(pref, i1, i2, start, 4, max_iterations=0, min_valid=64 * (n3 + 1))
    assert lv[0, 3]["flags"] == U.FEW_PIXELS


def _kink_free_point(seed, level):
    """tests/test_photo_align_cpu.py's point in units of the level's pixels: offsets 2^L (0.5 +- 0.3) px, so that every pixel of level L samples within
    0.2 .. 0.8 of a cell of the level-L img2 (up to the perspective term), and a move of 1e-3 px takes no sample across a cell border"""
    return (0.5 + (uniform01(seed, 4004, 8).astype(np.float64) * 2.0 - 1.0) * 0.3) * (1 << level)


@pytest.mark.parametrize("level", [0, 1, 2, 3])
@pytest.mark.parametrize("kind,seed", [("smooth", 1), ("stock", 2), ("smooth", 5), ("stock", 11)])
def test_level_gradient_is_the_derivative_of_the_level_cost(pref, kind, seed, level):
    """per level, g (full-resolution pixels) equals the central differences of the level's sum r^2 / 2 in each of the 8 offsets, step 1e-3 px, at 1e-5 of
    max |g|, on the float64 twin of the level's quantity at a point where no sample crosses a cell border and n_valid is equal at x +- step; and the
    fp32 quantity's g agrees with the twin's within the existing test's 3.5e-4 of max |g| (the method and both gates of
    tests/test_photo_align_cpu.py::test_gradient_is_the_derivative_of_the_cost)"""
    i1, i2 = (U.smooth_pair(seed, 2.0) if kind == "smooth" else U.stock_pair(seed))[:2]
    x = _kink_free_point(seed, level)
    _, g, n = P.ref_cost64(pref, i1, i2, x, level)
    fd = np.zeros(8)
    for k in range(8):
        e = np.zeros(8)
        e[k] = 1e-3
        cp, _, n_p = P.ref_cost64(pref, i1, i2, x + e, level)
        cm, _, n_m = P.ref_cost64(pref, i1, i2, x - e, level)
        assert n_p == n_m == n == (P.LEVEL_W[level] - 1) * (P.LEVEL_H[level] - 1)
        fd[k] = (cp - cm) / 2e-3
    rel = np.abs(fd - g).max() / np.abs(g).max()
    sums, ok = P.ref_sums(pref, i1, i2, x.astype(np.float32), level)
    _, g32 = U.ref_reduce(pref, x.astype(np.float32), sums)
    rel32 = np.abs(g32[0] - g).max() / np.abs(g).max()
    print(f"level {level} {kind} {seed}: |fd - g| / max |g| = {rel:.2e}; fp32 quantity vs float64 twin {rel32:.2e}")
    assert ok[0] == 1 and sums["n_valid"][0] == n
    assert rel < 1e-5
    assert rel32 < 3.5e-4


def test_photo_align_pyr_check_under_asan_ubsan(tmp_path):
    """the reference core on its fixed scene, the hostile starts and the four basin cases (passed in a file) under AddressSanitizer + UBSan: a stand-alone
    program; nothing loaded into python is sanitized"""
    exe, cases = str(tmp_path / "photo_align_pyr_check_san.bin"), str(tmp_path / "cases.bin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *U.HOST_FLAGS,
                    os.path.join(ROOT, "tests", "cpp", "photo_align_pyr_check.cpp"), "-o", exe], check=True)
    i1, i2, truth = P.basin_cases(32.0)
    with open(cases, "wb") as f:
        f.write(struct.pack("<iiif", 4, 4, 8, BASIN_GATE_PX))
        f.write(np.ascontiguousarray(i1, np.uint8).tobytes() + np.ascontiguousarray(i2, np.uint8).tobytes() + np.ascontiguousarray(truth, np.float64).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, cases], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "photo_align_pyr_check: ok" in r.stdout and r.stdout.count("basin case") == 4
