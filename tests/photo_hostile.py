"""What the CPU and the GPU tests of the photometric path on hostile inputs share: the frame pairs, the pool of candidate offsets, the
alignment's starts and option cases with the traces the host references gave for them, and the references' two extra entry points behind ctypes
(photo_ref_homography, photo_align_ref_edge)."""
import ctypes as C
import functools

import numpy as np

import photo_align_util as U

NPIX = 224 * 320
P4 = np.array([0, 0, 0, 223, 319, 223, 319, 0], np.float32)
PHOTO_DEGENERATE = 1                      # hnet_photo_residual.flags
CONVERGED, SINGULAR, DEGENERATE, FEW_PIXELS = U.CONVERGED, U.SINGULAR, U.DEGENERATE, U.FEW_PIXELS
ONE_1E30 = 0           # the component of `1e30one`: ul u
TWO_3E38 = [0, 1]      # the two components of `3e38`: ul u and v


@functools.lru_cache(maxsize=None)
def pairs():
    """the frame pairs, each 224 x 320 u8: {name: (img1, img2)}"""
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 256, (224, 320), dtype=np.uint8)
    checker = (np.random.default_rng(7).integers(0, 2, (224, 320), dtype=np.uint8) * 255).astype(np.uint8)
    return {"smooth": U.smooth_pair(1, 2.0)[:2], "smooth8": U.smooth_pair(1, 8.0)[:2],
            "noise": (noise, np.roll(noise, (1, 2), axis=(0, 1))),
            "checker": (checker, np.roll(checker, (0, 1), axis=(0, 1))),
            "black_white": (np.zeros((224, 320), np.uint8), np.full((224, 320), 255, np.uint8))}


def _quad(target):
    """the offsets that take the image corners (ul bl br ur) to `target` [8], on the grid of 2^-10 px"""
    t = np.round(np.asarray(target, np.float64) * 1024.0) / 1024.0
    return (t - P4).astype(np.float32)


def _shift(du, dv):
    return np.tile(np.array([du, dv], np.float32), 4)


def _one(k, value):
    o = np.zeros(8, np.float32)
    o[np.atleast_1d(k)] = value
    return o


@functools.lru_cache(maxsize=None)
def pool():
    """the candidate offsets: (names [19], offsets f32 [19, 8]).  Every finite component is a multiple of 2^-10 px below 2^20 in magnitude (the three huge
    ones apart), so that the corners p4 + offsets are exact in fp32 and the products inside dlt_solve are exact in a double: FMA contraction on the device
    cannot move H off the host's bits except at a rounding tie."""
    p4 = P4.astype(np.float64)
    c = {}
    c["zero"] = np.zeros(8, np.float32)
    c["line"] = _quad([0, 0, 10, 5, 20, 10, 30, 15])
    c["nan"] = np.full(8, np.nan, np.float32)
    c["nan1"] = _one(3, np.nan)
    c["inf"] = _one(3, np.inf)
    c["1e30all"] = np.full(8, 1e30, np.float32)
    c["1e30one"] = _one(ONE_1E30, 1e30)
    c["3e38"] = _one(TWO_3E38, 3e38)
    c["bowtie"] = _quad([319, 0, 0, 223, 319, 223, 0, 0])               # ul and ur targets swapped
    c["concave"] = _quad([0, 0, 0, 223, 319 - 250, 223 - 170, 319, 0])   # br moved by (-250, -170)
    c["far"] = _shift(400, 0)
    c["farneg"] = _shift(-5000, -5000)
    c["shift+1"] = _shift(1, 0)
    c["half-"] = _shift(-0.5, -0.5)
    c["half+"] = _shift(0.5, 0.5)
    c["collapse"] = _quad([100, 100] * 4)
    c["shrink"] = _quad(0.05 * p4 + 100)
    c["zoom3"] = _quad(3 * p4 - 300)
    c["flip"] = _quad([319, 223, 319, 0, 0, 0, 0, 223])                  # the rectangle rotated by 180 degrees
    names = list(c)
    off = np.stack([c[k] for k in names])
    fin = off[np.isfinite(off) & (np.abs(off) < 1e29)].astype(np.float64)
    assert len(names) == 19 and (fin * 1024 == np.round(fin * 1024)).all() and (np.abs(fin) < 2 ** 20).all()
    return names, off


def cand(name):
    names, off = pool()
    return off[names.index(name)]


# ---- residual records on `smooth` (tests/cpp/photo_ref.cpp, measured with the committed reference): name -> (flags, n_inside, n_edge)
RECORDS_SMOOTH = {
    "zero": (0, 71680, 0), "line": (1, 0, 0), "nan": (1, 0, 0), "nan1": (1, 0, 0), "inf": (1, 0, 0), "1e30all": (1, 0, 0), "collapse": (1, 0, 0),
    "1e30one": (0, 35896, 0), "3e38": (0, 24146, 0), "bowtie": (0, 640, 0), "concave": (0, 41986, 1), "far": (0, 0, 0), "farneg": (0, 0, 0),
    "shift+1": (0, 71456, 0), "half-": (0, 71456, 543), "half+": (0, 71137, 543), "shrink": (0, 71680, 0), "flip": (0, 71680, 0), "zoom3": (0, 8025, 0)}
SUM_ZERO_IMAGE_SMOOTH = 9.37138e6         # sum of img1 of `smooth`, six digits: the record's sum when every sample is 0

# ---- alignment starts on `smooth`, min_valid = 0 (tests/cpp/photo_align_ref.cpp): (name, start offsets, n_valid0 at K = 0, flags at K = 0)
def align_starts():
    s = [("shift(1,0)", _shift(1, 0), 223 * 318, 0), ("shift(0,1)", _shift(0, 1), 222 * 319, 0), ("shift(-1,-1)", _shift(-1, -1), 71137, 0),
         ("shift(310,0)", _shift(310, 0), 2007, 0), ("shift(318,0)", _shift(318, 0), 223, SINGULAR), ("shift(0,222)", _shift(0, 222), 319, SINGULAR),
         ("shift(319,0)", _shift(319, 0), 0, FEW_PIXELS), ("shift(0,223)", _shift(0, 223), 0, FEW_PIXELS)]
    for name, n0, fl in (("nan", 0, DEGENERATE), ("inf", 0, DEGENERATE), ("1e30all", 0, DEGENERATE), ("1e30one", 0, FEW_PIXELS), ("3e38", 23941, SINGULAR),
                         ("bowtie", 639, 0)):
        s.append((name, cand(name), n0, fl))
    return s


# ---- option and pair cases of the Levenberg-Marquardt loop, each from zero offsets: (name, pair, options, expected)
# expected: flags, trials, accepted (, lambda (relative 1e-12: a product of powers of ten), n_valid, unmoved: the offsets are bitwise the start's)
def step_cases():
    full = 223 * 319
    return [
        ("default-K10", "smooth", dict(max_iterations=10), dict(flags=0, trials=10, accepted=3, lam=10.0)),
        ("eps0", "smooth", dict(max_iterations=10, eps_px=0.0), dict(flags=0, trials=10, accepted=3, lam=10.0)),
        ("eps100", "smooth", dict(max_iterations=10, eps_px=100.0), dict(flags=CONVERGED, trials=1, accepted=1)),
        ("lambda1e3", "smooth", dict(max_iterations=10, lambda0=1e3), dict(flags=CONVERGED, trials=8, accepted=8)),
        ("lambda1e-300", "smooth", dict(max_iterations=10, lambda0=1e-300), dict(flags=0, trials=10, accepted=3, lam=1e-296)),
        ("lambda1e100", "smooth", dict(max_iterations=32, lambda0=1e100), dict(flags=0, trials=32, accepted=0, lam=1e132, unmoved=True)),
        ("min_valid+1", "smooth", dict(min_valid=full + 1), dict(flags=FEW_PIXELS, trials=0, accepted=0, unmoved=True)),
        ("min_valid=all", "smooth", dict(min_valid=full), dict(flags=0, trials=6, accepted=3)),
        ("count-refused-K6", "smooth8", dict(max_iterations=6, min_valid=71137), dict(flags=0, trials=6, accepted=0, lam=1e3, unmoved=True)),
        ("count-refused-K32", "smooth8", dict(max_iterations=32, min_valid=71137), dict(flags=CONVERGED, trials=10, accepted=1)),
        ("count-70500", "smooth8", dict(max_iterations=32, min_valid=70500), dict(trials=29, accepted=11, n_valid=70500)),
        ("noise", "noise", dict(max_iterations=6), dict(flags=CONVERGED, trials=5, accepted=5)),
        ("checker", "checker", dict(max_iterations=10), dict(flags=CONVERGED)),
        ("black_white", "black_white", dict(), dict(flags=SINGULAR, trials=0, accepted=0, unmoved=True)),
    ]


OVERFLOW_LAMBDA0 = (1e280, 1e290, 1e300)   # were legal and ended SINGULAR when lambda overflowed; refused since lambda0 is capped at 1e100


def check_trace(rec, want, name):
    """the asserted part of a step case's record (host reference and device alike)"""
    for k in ("flags", "trials", "accepted", "n_valid"):
        if k in want:
            assert rec[k] == want[k], (name, k, rec[k], want[k])
    if "lam" in want:
        assert abs(rec["lambda"] - want["lam"]) <= 1e-12 * want["lam"], (name, rec["lambda"])
    if want.get("unmoved"):
        assert rec["offsets_px"].tobytes() == np.zeros(8, np.float32).tobytes(), name
    assert rec["accepted"] <= rec["trials"]


def ref_homography(pref, offsets):
    """photo_ref_homography -> (H f32 [n, 9], ok [n])"""
    off = np.ascontiguousarray(offsets, np.float32).reshape(-1, 8)
    h, ok = np.zeros((off.shape[0], 9), np.float32), np.zeros(off.shape[0], np.int32)
    pref.photo_ref_homography(off.shape[0], C.c_void_p(off.ctypes.data), C.c_void_p(h.ctypes.data), C.c_void_p(ok.ctypes.data))
    return h, ok


def ref_edge(aref, offsets):
    """photo_align_ref_edge -> n_edge [n]: the pixels within 1e-3 px of a bound of VALID"""
    off = np.ascontiguousarray(offsets, np.float32).reshape(-1, 8)
    out = np.zeros(off.shape[0], np.int32)
    aref.photo_align_ref_edge(None, None, off.shape[0], C.c_void_p(off.ctypes.data), C.c_void_p(out.ctypes.data))
    return out


def ref_opts_valid(aref, **kw):
    o = U.opts(**kw)
    return bool(aref.photo_align_ref_opts_valid(C.byref(o)))
