"""The photometric path of the device on hostile inputs (csrc/kernels_photo.hip, csrc/kernels_photo_align.hip): quads without a homography,
with Z changing sign inside the image, offsets of 1e30 and NaN, candidates and starts exactly on the inside / valid bounds, images of maximal gradient, and
options under which the Levenberg-Marquardt loop refuses trial after trial - against the host references as test_photo_hostile_cpu.py pins them
(tests/photo_hostile.py holds the inputs).  Main model prior-3, N = 16, max_batch 9; every call is n <= 9."""
import ctypes as C

import numpy as np
import pytest

import photo_align_util as U
import photo_hostile as PH
import test_gpu_photo_align as TA
from test_photo_cpu import build_photo_ref, photo_ref_records

pytestmark = pytest.mark.gpu

INVALID = 1
NPIX = PH.NPIX
REC_PAIRS = ("smooth", "noise", "checker")
# Measured on an MI355X, device against the host reference tests/cpp/photo_ref.cpp over the 3 pairs x 19 candidates of test b. (printed by the test), each
# gated at 10 x the measurement and never above 1e-4.  Every map value has the host's bits, so what is left is the order of 71 680 additions in double:
#   worst |sum - reference sum| / reference sum: 2.657e-15
MEASURED_SUM_REL = 2.7e-15
#   worst (|sum_inside - reference sum_inside| - 255 |n_inside - reference n_inside|) / sum, floored at 0: 2.657e-15
MEASURED_SUM_INSIDE_REL = 2.7e-15
#   worst |n_inside - reference n_inside| over the pool and worst |n_valid0 - reference n_valid0| over the starts of test d.: measured 0 and 0.  The positions
#   have the host's bits, so no pixel changes sides, the 543 of half- / half+ and the 862 of the integer shifts that lie on a bound included; the
#   reference's n_edge stays the outer bound
MEASURED_DN_INSIDE = 0
MEASURED_DN_VALID = 0
# Test d. holds mse, grad and info to the sibling module's 10 x MEASURED_LIN for every start.  Measured there, worst relative difference from the host reference
# over K = 0 and K = 6: the shifts mse 2.1e-13, grad 3.5e-13, info 7.0e-13; 3e38 and bowtie (stated apart: the quad folds over or leaves fp32's comfortable
# range) mse 1.9e-14, grad 1.4e-14, info 1.3e-13: they need no gate of their own.


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return build_photo_ref(tmp_path_factory.mktemp("photo_ref_hostile_gpu"))


@pytest.fixture(scope="module")
def aref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp("photo_align_ref_hostile_gpu"))


@pytest.fixture(scope="module")
def eng(blob):
    from cuahn_vio_amd.homography_net import HnetEngine
    e = HnetEngine(blob, variant="prior3", mc_samples=16, dropout_p=0.05, mc_seed=9, max_batch=9)
    yield e
    e.close()


@pytest.fixture(scope="module")
def frames():
    p = PH.pairs()
    return np.stack([p[k][0] for k in REC_PAIRS]), np.stack([p[k][1] for k in REC_PAIRS])


@pytest.fixture(scope="module")
def pool_records(eng, pref, frames):
    """the device's records and maps of the pool on the 3 pairs in ONE call (n = 3, m = 19), and the host reference's, once for the module"""
    names, off = PH.pool()
    offs = np.repeat(off[None], 3, 0)
    rec, emap = eng.op_photo_residual(frames[0], frames[1], offs, want_map=True)
    ref, edge = photo_ref_records(pref, frames[0], frames[1], offs)
    return {"names": names, "off": off, "offs": offs, "rec": rec, "map": emap, "ref": ref, "edge": edge}


def _dev_homographies(eng, off):
    with np.errstate(invalid="ignore", over="ignore"):
        dst = (PH.P4[None] + off).astype(np.float32)
    return eng.op_dlt(dst).reshape(-1, 9)


def _ulp(a, b):
    """distance of two finite floats in units of the last place"""
    ia, ib = np.array([a, b], np.float32).view(np.int32).astype(np.int64)
    ia, ib = (ia if ia >= 0 else -(ia & 0x7FFFFFFF)), (ib if ib >= 0 else -(ib & 0x7FFFFFFF))
    return abs(int(ia) - int(ib))


def test_homographies_have_the_hosts_bits(eng, pref):
    """a. over the whole pool op_dlt(p4 + offsets) equals photo_ref_homography bit for bit where the host has a matrix, and has a non-finite entry exactly where
    the host has none"""
    names, off = PH.pool()
    href, ok = PH.ref_homography(pref, off)
    hdev = _dev_homographies(eng, off)
    bad = []
    for k, name in enumerate(names):
        finite = bool(np.isfinite(hdev[k]).all())
        assert finite == bool(ok[k]), (name, hdev[k])
        if finite and hdev[k].tobytes() != href[k].tobytes():
            bad += [(name, e, float(hdev[k, e]), float(href[k, e]), _ulp(hdev[k, e], href[k, e])) for e in range(9) if hdev[k, e] != href[k, e]]
    print("entries of H off the host's bits (candidate, entry, device, host, ulp):", bad)
    assert not bad


def test_records_on_the_pool(eng, pool_records, frames):
    """b. smooth, noise and checker x the 19 candidates in one call with the map: flags and the DEGENERATE set are the reference's.  DEGENERATE: nothing
    inside, every map value |0 - img1 / 255| * 255.  Others: the map is |op_warp(f2, H) - f1| * 255 bitwise, n_inside within the reference's n_edge (and
    within 10 x MEASURED_DN_INSIDE), sum_inside within 255 per differing pixel plus the measured tolerance.  Every sum is the map's float64 sum to 1e-10
    and the reference's to 10 x MEASURED_SUM_REL; where no rounding is involved (DEGENERATE, far, farneg) to 1e-10, with n_inside and sum_inside equal."""
    from oracle import pyoracle
    P = pool_records
    hs = _dev_homographies(eng, P["off"])
    worst = {"sum": 0.0, "sum_inside": 0.0, "dn": 0, "sum_vs_map": 0.0}
    fails = []
    for b, pair in enumerate(REC_PAIRS):
        f1, f2 = pyoracle.as_f32_image(frames[0][b]), pyoracle.as_f32_image(frames[1][b])
        for c, name in enumerate(P["names"]):
            r, w, edge, m = P["rec"][b, c], P["ref"][b, c], int(P["edge"][b, c]), P["map"][b, c]
            assert r["flags"] == w["flags"], (pair, name, r["flags"])
            assert np.isfinite(m).all() and np.isfinite(r["sum"]) and np.isfinite(r["sum_inside"]), (pair, name)
            if pair == "smooth":
                assert (w["flags"], w["n_inside"], edge) == PH.RECORDS_SMOOTH[name], name
            msum = float(m.astype(np.float64).sum())
            assert abs(r["sum"] - msum) <= 1e-10 * msum, (pair, name)
            worst["sum_vs_map"] = max(worst["sum_vs_map"], abs(r["sum"] - msum) / msum)
            if r["flags"] == PH.PHOTO_DEGENERATE:
                want = np.abs(np.float32(0.0) - f1) * np.float32(255)
                assert r["n_inside"] == 0 and r["sum_inside"] == 0.0, (pair, name)
            else:
                want = np.abs(eng.op_warp(f2, hs[c]) - f1) * np.float32(255)
            assert want.dtype == np.float32 and m.tobytes() == want.tobytes(), (pair, name)
            dn = abs(int(r["n_inside"]) - int(w["n_inside"]))
            ds = abs(r["sum_inside"] - w["sum_inside"])
            rel = abs(r["sum"] - w["sum"]) / w["sum"]
            rel_in = max(ds - 255.0 * dn, 0.0) / r["sum"]
            print(f"{pair} {name}: n_inside {r['n_inside']} (reference {w['n_inside']}, n_edge {edge}), |d sum| / sum {rel:.3e}, |d sum_inside| {ds:.3e} "
                  f"({rel_in:.3e} of sum beyond 255 dn)")
            if r["flags"] == PH.PHOTO_DEGENERATE or name in ("far", "farneg"):
                assert rel <= 1e-10 and r["n_inside"] == w["n_inside"] == 0 and r["sum_inside"] == w["sum_inside"] == 0.0, (pair, name)
                continue
            worst["sum"], worst["sum_inside"], worst["dn"] = max(worst["sum"], rel), max(worst["sum_inside"], rel_in), max(worst["dn"], dn)
            if not (dn <= edge and dn <= 10 * MEASURED_DN_INSIDE):
                fails.append((pair, name, "n_inside", dn, edge))
            if not ds <= 255.0 * dn + min(10 * MEASURED_SUM_INSIDE_REL, 1e-4) * r["sum"]:
                fails.append((pair, name, "sum_inside", ds, dn))
            if not rel <= min(10 * MEASURED_SUM_REL, 1e-4):
                fails.append((pair, name, "sum", rel))
    print("pool, device vs host reference, worst:", {k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in worst.items()})
    assert not fails, fails


def test_neighbours_do_not_leak(eng, pool_records, frames):
    """c. the `zero` candidate's record is bitwise the same alone (m = 1), in slot 0 of the m = 19 call and in slot 0 of an m = 66 call whose other 65 slots
    alternate `nan` and `line`; the `nan` in slot 65, the last lane that forms a matrix, is DEGENERATE with the reference's sum; and the m = 19 call without
    the map returns the same bytes"""
    P = pool_records
    zero, nan, line = PH.cand("zero"), PH.cand("nan"), PH.cand("line")
    alone = eng.op_photo_residual(frames[0], frames[1], np.repeat(zero[None, None], 3, 0))
    crowd = np.stack([zero] + [nan if k % 2 else line for k in range(1, 66)])
    assert np.isnan(crowd[65]).all() and not np.isnan(crowd[64]).any()
    big = eng.op_photo_residual(frames[0], frames[1], np.repeat(crowd[None], 3, 0))
    names = P["names"]
    for b, pair in enumerate(REC_PAIRS):
        assert alone[b, 0].tobytes() == P["rec"][b, 0].tobytes() == big[b, 0].tobytes(), pair
        assert alone[b, 0]["flags"] == 0 and alone[b, 0]["n_inside"] == NPIX
        assert (big["flags"][b, 1:] == PH.PHOTO_DEGENERATE).all() and not big["n_inside"][b, 1:].any() and not big["sum_inside"][b, 1:].any()
        want = P["ref"][b, names.index("nan")]["sum"]
        assert abs(big[b, 65]["sum"] - want) <= 1e-10 * want, pair
        assert len({big[b, k].tobytes() for k in range(1, 66)}) == 1                       # (every degenerate slot: the same record)
        assert big[b, 65].tobytes() == P["rec"][b, names.index("nan")].tobytes() == P["rec"][b, names.index("line")].tobytes()
    assert eng.op_photo_residual(frames[0], frames[1], P["offs"]).tobytes() == P["rec"].tobytes()


def _finite(rec, name):
    for f in ("mse0", "mse", "lambda", "grad", "info"):
        assert np.isfinite(rec[f]).all(), (name, f)


def _lin_close(d, r, gate, name, fails):
    got = {"mse": abs(d["mse"] - r["mse"]) / r["mse"] if r["mse"] else abs(d["mse"]), "grad": TA._rel(d["grad"], r["grad"]) if r["grad"].any() else 0.0,
           "info": TA._rel(d["info"], r["info"])}
    for k, v in got.items():
        if not v <= 10 * gate[k]:
            fails.append((name, k, v))
    return got


def test_alignment_starts(eng, aref):
    """d. the starts of test_photo_hostile_cpu.py on `smooth` with min_valid = 0 (on and beyond the valid bound, NaN, inf, 1e30, 3e38, the bowtie) in calls of at
    most 9, at K = 0 and at K = 6: flags, trials and accepted are the reference's; n_valid0 is equal where no pixel lies within 1e-3 px of a bound, within
    the reference's n_edge otherwise (and within 10 x MEASURED_DN_VALID); starts that stop at once come back bit for bit, a NaN's payload included;
    DEGENERATE and FEW_PIXELS have info = grad = 0 and mse0 = mse = 0; nothing is non-finite; where flags is 0, or SINGULAR with a non-zero info, mse, grad
    and info lie within 10 x MEASURED_LIN of the reference, 3e38 and the bowtie included.  (A CONVERGED record is left out of that gate: at a minimum grad
    is what remains of 71 137 cancelling terms, and its relative difference measures the cancellation, 1.1e-11 on shift(-1,-1), not the kernel.)"""
    i1, i2 = PH.pairs()["smooth"]
    starts = PH.align_starts()
    payload = PH.cand("nan").copy()
    payload.view(np.uint32)[:] = 0x7FC12345
    starts.append(("nan-payload", payload, 0, PH.DEGENERATE))
    off = np.stack([s[1] for s in starts])
    n = len(starts)
    a, b = np.repeat(i1[None], n, 0), np.repeat(i2[None], n, 0)
    edge = PH.ref_edge(aref, off)
    fails, worst, worst_folded, worst_dn = [], dict.fromkeys(TA.MEASURED_LIN, 0.0), dict.fromkeys(TA.MEASURED_LIN, 0.0), 0
    for K in (0, 6):
        dev = np.concatenate([eng.op_photo_align(a[s:e], b[s:e], off[s:e], max_iterations=K, min_valid=0) for s, e in ((0, 9), (9, n))])
        ref = U.ref_run(aref, a, b, off, max_iterations=K, min_valid=0)
        for k, (name, x0, n0, flags0) in enumerate(starts):
            d, r = dev[k], ref[k]
            dn = abs(int(d["n_valid0"]) - int(r["n_valid0"]))
            worst_dn = max(worst_dn, dn)
            print(f"{name} K={K}: flags {d['flags']}, trials {d['trials']}, accepted {d['accepted']}, n_valid0 {d['n_valid0']} (reference {r['n_valid0']}, "
                  f"n_edge {edge[k]}), n_valid {d['n_valid']} (reference {r['n_valid']})")
            assert (d["flags"], d["trials"], d["accepted"]) == (r["flags"], r["trials"], r["accepted"]), (name, K)
            if K == 0:
                assert (r["n_valid0"], r["flags"]) == (n0, flags0), name
            if not (dn <= edge[k] and dn <= 10 * MEASURED_DN_VALID):
                fails.append((name, K, "n_valid0", int(d["n_valid0"]), int(r["n_valid0"]), int(edge[k])))
            _finite(d, name)
            if d["trials"] == 0 or d["accepted"] == 0:
                assert d["offsets_px"].tobytes() == x0.tobytes(), (name, K)
            if d["flags"] in (PH.DEGENERATE, PH.FEW_PIXELS):
                assert not d["info"].any() and not d["grad"].any() and d["mse0"] == 0.0 and d["mse"] == 0.0 and d["trials"] == 0, (name, K)
            elif d["flags"] == 0 or (d["flags"] == PH.SINGULAR and d["info"].any()):
                folded = name in ("3e38", "bowtie")
                got = _lin_close(d, r, TA.MEASURED_LIN, f"{name} K={K}", fails)
                print(f"    vs reference: " + ", ".join(f"{f} {v:.3e}" for f, v in got.items()))
                w = worst_folded if folded else worst
                for f, v in got.items():
                    w[f] = max(w[f], v)
                diff = float(np.abs(d["offsets_px"].astype(np.float64) - r["offsets_px"]).max())
                if not diff <= max(10 * TA.MEASURED_OFFSETS_PX, TA.OFFSET_ULP_PX):
                    fails.append((name, K, "offsets", diff))
    print("starts, device vs host reference, worst relative difference:", {k: f"{v:.3e}" for k, v in worst.items()}, "; 3e38 and bowtie:",
          {k: f"{v:.3e}" for k, v in worst_folded.items()}, f"; worst |d n_valid0| {worst_dn}")
    assert not fails, fails
    d = eng.op_photo_align(i1, i2, PH.cand("bowtie"), max_iterations=6)[0]                    # the default min_valid
    assert d["flags"] == PH.FEW_PIXELS and d["trials"] == 0 and not d["info"].any() and abs(int(d["n_valid0"]) - 639) <= 10 * MEASURED_DN_VALID


@pytest.fixture(scope="module")
def step_refs(aref):
    p = PH.pairs()
    return {name: U.ref_run(aref, p[pair][0], p[pair][1], np.zeros(8, np.float32), **o)[0] for name, pair, o, _want in PH.step_cases()}


@pytest.mark.parametrize("case", PH.step_cases(), ids=[c[0] for c in PH.step_cases()])
def test_steps(eng, step_refs, case):
    """e. every option and pair case of test_photo_hostile_cpu.py on the device: flags, trials, accepted, n_valid0 and n_valid are the reference's (a decision
    that differs shows here: mse < rec.mse, or the count), lambda is the same double, and the final offsets lie within max(10 x MEASURED_OFFSETS_PX, one
    ulp of an offset) of the reference's"""
    name, pair, o, want = case
    p = PH.pairs()[pair]
    d, r = eng.op_photo_align(p[0], p[1], np.zeros(8, np.float32), **o)[0], step_refs[name]
    diff = float(np.abs(d["offsets_px"].astype(np.float64) - r["offsets_px"]).max())
    print(f"{name}: flags {d['flags']} / {r['flags']}, trials {d['trials']} / {r['trials']}, accepted {d['accepted']} / {r['accepted']}, n_valid0 {d['n_valid0']} / "
          f"{r['n_valid0']}, n_valid {d['n_valid']} / {r['n_valid']}, lambda {d['lambda']:.17g} / {r['lambda']:.17g}, mse {d['mse']:.9g} / {r['mse']:.9g}, "
          f"|d offsets| {diff:.3e} px")
    for f in ("flags", "trials", "accepted", "n_valid0", "n_valid"):
        assert d[f] == r[f], (name, f, d[f], r[f])
    assert d["lambda"] == r["lambda"], name
    assert diff <= max(10 * TA.MEASURED_OFFSETS_PX, TA.OFFSET_ULP_PX), name
    PH.check_trace(d, want, name)
    _finite(d, name)
    assert d["mse"] <= d["mse0"]


def test_damping_cannot_overflow_on_device(eng):
    """lambda0 = 1e280, 1e290 and 1e300 (SINGULAR on a healthy pair before the cap, when lambda overflowed) are refused and write nothing; 1e100 is legal"""
    from cuahn_vio_amd import _capi
    i1, i2 = PH.pairs()["smooth"]
    L = _capi.lib()
    out = np.full(_capi.PHOTO_ALIGN_DTYPE.itemsize, 0xA5, np.uint8)
    keep = out.copy()
    x0 = np.zeros(8, np.float32)
    a, b = np.ascontiguousarray(i1), np.ascontiguousarray(i2)
    for lam in PH.OVERFLOW_LAMBDA0 + (1.0000001e100, float("inf"), float("nan")):
        o = _capi.photo_align_opts(max_iterations=32, lambda0=lam)
        assert L.hnet_op_photo_align(eng.handle, a.ctypes.data, b.ctypes.data, 1, x0.ctypes.data, C.addressof(o), out.ctypes.data) == INVALID, lam
        assert out.tobytes() == keep.tobytes()
    o = _capi.photo_align_opts(max_iterations=0, lambda0=1e100)
    assert L.hnet_op_photo_align(eng.handle, a.ctypes.data, b.ctypes.data, 1, x0.ctypes.data, C.addressof(o), out.ctypes.data) == 0
    assert out.view(_capi.PHOTO_ALIGN_DTYPE)[0]["flags"] == 0


def test_early_stop_keeps_its_bits_beside_32_trials(eng, aref):
    """e. the `rec[pair].flags != 0` early return of both kernels across 32 launch pairs.  K = 32, eps_px = 100, lambda0 = 1e-30, min_valid = 71137: `smooth` is
    CONVERGED after its first trial, a NaN start is DEGENERATE before any, and `smooth8` beside them is refused 32 times (every improving trial loses
    pixels, and lambda has not grown enough by then for a step too small to lose one).  The two that stopped have the bytes they have alone."""
    p = PH.pairs()
    i1 = np.stack([p["smooth"][0], p["smooth8"][0], p["smooth"][0]])
    i2 = np.stack([p["smooth"][1], p["smooth8"][1], p["smooth"][1]])
    x0 = np.stack([np.zeros(8, np.float32), np.zeros(8, np.float32), PH.cand("nan")])
    o = dict(max_iterations=32, eps_px=100.0, lambda0=1e-30, min_valid=71137)
    three = eng.op_photo_align(i1, i2, x0, **o)
    ref = U.ref_run(aref, i1, i2, x0, **o)
    assert [(r["flags"], r["trials"], r["accepted"]) for r in three] == [(PH.CONVERGED, 1, 1), (0, 32, 0), (PH.DEGENERATE, 0, 0)]
    for k in range(3):
        assert (three[k]["flags"], three[k]["trials"], three[k]["accepted"], three[k]["lambda"]) == (ref[k]["flags"], ref[k]["trials"], ref[k]["accepted"],
                                                                                                     ref[k]["lambda"]), k
        assert eng.op_photo_align(i1[k], i2[k], x0[k], **o)[0].tobytes() == three[k].tobytes(), k
    order = [1, 2, 0]                                                        # the pair that runs on in slot 0
    assert eng.op_photo_align(i1[order], i2[order], x0[order], **o).tobytes() == three[order].tobytes()
