"""The photometric path on hostile inputs, on the CPU: the host references tests/cpp/photo_ref.cpp and tests/cpp/photo_align_ref.cpp pinned on
the pool of tests/photo_hostile.py - quads without a homography, with Z changing sign inside the image, offsets of 1e30, candidates on the inside
bound - and on the options, starts and frame pairs that make the Levenberg-Marquardt loop refuse: what test_gpu_photo_hostile.py holds the device
against.  Every number asserted here was measured with the committed references."""
import numpy as np
import pytest

import photo_align_util as U
import photo_hostile as PH
from test_photo_cpu import build_photo_ref, photo_ref_records


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return build_photo_ref(tmp_path_factory.mktemp("photo_ref_hostile"))


@pytest.fixture(scope="module")
def aref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp("photo_align_ref_hostile"))


def _finite(rec, name):
    for f in ("mse0", "mse", "lambda", "grad", "info"):
        assert np.isfinite(rec[f]).all(), (name, f)


def test_records_on_the_pool(pref):
    """flags, n_inside and n_edge of the 19 candidates on `smooth` are the table's; a record without a homography or without a pixel inside carries the sum
    of img1 (every sample 0) and sum_inside = 0; n_edge, which bounds what the device may differ by, stays below 1 % of the pixels in every case (at most
    543 of 71 680, the 320 + 224 - 1 pixels of a row and a column on the bound)"""
    names, off = PH.pool()
    i1, i2 = PH.pairs()["smooth"]
    rec, edge = photo_ref_records(pref, i1, i2, off[None])
    all1 = float(i1.astype(np.int64).sum())
    assert abs(all1 - PH.SUM_ZERO_IMAGE_SMOOTH) <= 0.5e-5 * all1
    for k, name in enumerate(names):
        r = rec[0, k]
        print(f"{name}: flags {r['flags']}, n_inside {r['n_inside']}, n_edge {edge[0, k]}, sum {r['sum']:.6f}, sum_inside {r['sum_inside']:.6f}")
        assert (r["flags"], r["n_inside"], edge[0, k]) == PH.RECORDS_SMOOTH[name], name
        assert np.isfinite(r["sum"]) and np.isfinite(r["sum_inside"]) and 0.0 <= r["sum_inside"] <= r["sum"]
        if r["flags"] == PH.PHOTO_DEGENERATE or r["n_inside"] == 0:
            assert r["sum"] == all1 and r["sum_inside"] == 0.0 and r["n_inside"] == 0, name
        assert edge[0, k] <= PH.NPIX // 100, name
    assert edge.max() == 543


def test_no_position_lies_exactly_on_the_inside_bound():
    """Why `half-` and `half+` have 543 pixels NEAR the inside bound and none ON it: the sampler un-normalises ix = ((g + 1) * 0.5) * 319 from an fp32 g, and
    near g = -(1 + 1 / 319) the sum g + 1 is a multiple of 2^-23, so ix is 319 m 2^-24 exactly (m < 2^15: the product is exact) and never -0.5: 319 = 11 * 29
    divides no power of two.  The same holds for iy with 223.  Every fp32 g within 1e-4 of the bound is enumerated; the nearest positions are 8.0e-6 px (ix)
    and 1.0e-6 px (iy) away.  So `-0.5 < ix` and `-0.5 <= ix` select the same pixels for every input: no test can tell them apart, and none tries.  The upper bound is
    different - near 319.5 the product is rounded to a grid of 2^-15 px that holds 319.5 (printed, not asserted) - and so are the bounds of VALID: g = -1 and g = 1 give ix = 0
    and 319 exactly (shift starts put whole columns there)."""
    one, half = np.float32(1.0), np.float32(0.5)
    for size in (320, 224):
        scale = np.float32(size - 1)
        for bound in (-0.5, size - 0.5):
            g0 = np.float32(2.0 * bound / (size - 1) - 1.0)
            lo = np.array([g0 - np.float32(1e-4)], np.float32).view(np.int32)[0]
            hi = np.array([g0 + np.float32(1e-4)], np.float32).view(np.int32)[0]
            g = np.arange(min(lo, hi), max(lo, hi) + 1, dtype=np.int32).view(np.float32)
            pos = ((g + one) * half) * scale
            assert pos.dtype == np.float32 and len(g) > 800 and pos.min() < bound < pos.max()
            gap = np.abs(pos.astype(np.float64) - bound).min()
            print(f"size {size}, bound {bound}: {len(g)} values of g, nearest position {gap:.2e} px away")
            if bound < 0:
                assert gap > 0.0
        for gv, want in ((-1.0, 0.0), (1.0, float(size - 1))):
            assert ((np.float32(gv) + one) * half) * scale == np.float32(want)


def test_homographies_of_the_pool(pref):
    """photo_ref_homography: no matrix for exactly the candidates the records call DEGENERATE, all NaN there, and nine finite floats with h33 = 1 elsewhere"""
    names, off = PH.pool()
    h, ok = PH.ref_homography(pref, off)
    for k, name in enumerate(names):
        assert bool(ok[k]) == (PH.RECORDS_SMOOTH[name][0] == 0), name
        assert np.isfinite(h[k]).all() and h[k, 8] == 1.0 if ok[k] else np.isnan(h[k]).all(), name
    assert h[names.index("zero")].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1]


def test_alignment_starts(aref):
    """K = 0 on `smooth` with min_valid = 0: the table's n_valid0 and flags at starts on and beyond the valid bound and at non-finite and enormous offsets;
    DEGENERATE starts come back bit for bit, NaN payload included; bowtie makes 6 trials at K = 6 and is FEW_PIXELS at the default min_valid"""
    i1, i2 = PH.pairs()["smooth"]
    starts = PH.align_starts()
    off = np.stack([s[1] for s in starts])
    n = len(starts)
    rec = U.ref_run(aref, np.repeat(i1[None], n, 0), np.repeat(i2[None], n, 0), off, max_iterations=0, min_valid=0)
    edge = PH.ref_edge(aref, off)
    for b, (name, x0, n0, flags) in enumerate(starts):
        r = rec[b]
        print(f"{name}: n_valid0 {r['n_valid0']}, flags {r['flags']}, n_edge {edge[b]}")
        assert (r["n_valid0"], r["flags"]) == (n0, flags), name
        assert r["trials"] == 0 and r["accepted"] == 0 and r["offsets_px"].tobytes() == x0.tobytes(), name
        _finite(r, name)
        if flags in (PH.DEGENERATE, PH.FEW_PIXELS):
            assert not r["info"].any() and not r["grad"].any() and r["mse0"] == 0.0 and r["mse"] == 0.0
    nan = PH.cand("nan").copy()
    nan.view(np.uint32)[:] = 0x7FC12345                                      # a payload of its own
    r = U.ref_run(aref, i1, i2, nan, max_iterations=6, min_valid=0)[0]
    assert r["flags"] == PH.DEGENERATE and r["offsets_px"].tobytes() == nan.tobytes()
    r = U.ref_run(aref, i1, i2, PH.cand("bowtie"), max_iterations=6, min_valid=0)[0]
    assert (r["n_valid0"], r["flags"], r["trials"], r["accepted"]) == (639, 0, 6, 1)
    _finite(r, "bowtie")
    r = U.ref_run(aref, i1, i2, PH.cand("bowtie"), max_iterations=6)[0]
    assert r["flags"] == PH.FEW_PIXELS and r["n_valid0"] == 639 and r["trials"] == 0


@pytest.fixture(scope="module")
def traces(aref):
    """the host reference on every step case, once for the module"""
    p = PH.pairs()
    return {name: U.ref_run(aref, p[pair][0], p[pair][1], np.zeros(8, np.float32), **o)[0] for name, pair, o, _want in PH.step_cases()}


@pytest.mark.parametrize("case", PH.step_cases(), ids=[c[0] for c in PH.step_cases()])
def test_steps(traces, case):
    """the whole trace of every option and pair case: trials, accepted, flags, lambda, and no non-finite number in any record"""
    name, _pair, o, want = case
    r = traces[name]
    print(f"{name}: flags {r['flags']}, trials {r['trials']}, accepted {r['accepted']}, lambda {r['lambda']:.17g}, n_valid {r['n_valid0']} -> {r['n_valid']}, "
          f"mse {r['mse0']:.6f} -> {r['mse']:.6f}, offsets {r['offsets_px'].tolist()}")
    PH.check_trace(r, want, name)
    _finite(r, name)
    assert r["mse"] <= r["mse0"]


def test_steps_in_detail(traces, aref):
    """what the traces mean: eps_px = 0 never converges and leaves the default's record; lambda0 = 1e-300 the default's decisions; 32 refusals at lambda0 = 1e100
    leave lambda at 1e132 and flags 0 (the largest legal damping stays far from overflow); a trial refused for its COUNT (mse smaller, fewer pixels than
    min_valid) grows lambda until a step too small to lose a pixel is accepted: CONVERGED 8 px from the truth with mse == mse0 to six digits - the flag
    reports a small step, not a small residual"""
    d, e0, lo = traces["default-K10"], traces["eps0"], traces["lambda1e-300"]
    assert d.tobytes() == e0.tobytes()
    assert (lo["trials"], lo["accepted"], lo["flags"], lo["n_valid"]) == (d["trials"], d["accepted"], d["flags"], d["n_valid"])
    r = traces["count-refused-K32"]
    truth = U.smooth_pair(1, 8.0)[2]
    assert r["flags"] == PH.CONVERGED and r["lambda"] > 1e4 and 0 < (r["mse0"] - r["mse"]) <= 1e-6 * r["mse0"]
    assert np.abs(r["offsets_px"].astype(np.float64) - truth).max() > 7.0 and np.abs(r["offsets_px"]).max() < 1e-3
    assert r["n_valid"] == r["n_valid0"] == 71137
    r = traces["count-70500"]
    assert r["n_valid0"] == 71137 and r["mse"] < 0.5 * r["mse0"]
    r = traces["checker"]
    assert np.abs(r["offsets_px"].reshape(4, 2) - [1.0, 0.0]).max() < 1e-3 and r["mse"] < 1e-4
    r = traces["black_white"]
    assert not r["info"].any() and not r["grad"].any() and r["mse0"] == 255.0 ** 2 and r["n_valid0"] == 223 * 319
    r = traces["min_valid=all"]
    assert r["n_valid0"] == 223 * 319 and r["n_valid"] >= 223 * 319


def test_damping_cannot_overflow(aref):
    """lambda0 = 1e280, 1e290 and 1e300 were accepted and ended SINGULAR after 23, 13 and 3 refusals on a healthy pair, when A[j][j] + lambda A[j][j] overflowed
    in the damped factorisation; options above 1e100 are refused now (hnet_align::opts_valid), 1e100 itself is legal, and no legal call can take lambda past
    1e132, where diag(A) (2.4e5 on `smooth`) times lambda is 1e137"""
    for lam in PH.OVERFLOW_LAMBDA0 + (1.0000001e100, np.inf, np.nan, 0.0, -1.0):
        assert not PH.ref_opts_valid(aref, lambda0=lam), lam
    for lam in (1e100, 1e-300, 5e-324, 1e-3):
        assert PH.ref_opts_valid(aref, lambda0=lam), lam
    i1, i2 = PH.pairs()["smooth"]
    r = U.ref_run(aref, i1, i2, np.zeros(8, np.float32), max_iterations=0)[0]
    assert r["flags"] == 0 and 1e5 < r["info"].diagonal().max() < 1e6
    assert np.isfinite(r["info"].diagonal().max() * 1e100 * 10.0 ** 32)
