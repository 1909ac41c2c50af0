"""What the CPU and the GPU tests of the fine stage of the search and of the fine relocalisation share (include/hnet.h hnet_op_photo_search_fine,
hnet_sessions_keyframe_relocalise_fine): the tables, the hand-built cases on level-2 thumbnails, the gates on the rows, the host reference
tests/cpp/photo_search_fine_ref.cpp behind ctypes, a numpy restatement of the level-2 thumbnail, the warp, the masked sums, the order and the record, and
the record layouts."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import keyframe_util as K
import photo_align_util as U
import photo_search_oriented_util as O
import photo_search_util as S
from cuahn_vio_amd import _capi, synth

ROOT = U.ROOT
HYP, OREC = O.HYP, O.OREC
PART, FREC, FRELOC = _capi.PHOTO_SEARCH_FINE_PART_DTYPE, _capi.PHOTO_SEARCH_FINE_DTYPE, _capi.KEYFRAME_RELOC_FINE_DTYPE
assert PART.itemsize == 128 and FREC.itemsize == 288 and FRELOC.itemsize == 2168
FW, FH, NE, MAX_R = 80, 56, 9, 4
NAN32 = np.array([0x7FC00000] * 8, np.uint32)

# the two tables of the rows: (first_deg, step_deg, count) with n_fine 5 and radius 3
TABLE_60 = (-180.0, 6.0, 60)
TABLE_30 = (-180.0, 12.0, 30)
# The gates on the final start of the yawed rows (worst corner component against the truth, px): TWICE the worst the host reference measures over seeds
# 1, 2, 5, 11 x YAW_ROWS, as tests/test_photo_search_fine_cpu.py::test_the_yawed_rows prints it.  The issue's numpy prototype measured 4.40 / 5.02 px.
FINE_START_60 = 4.40
FINE_START_30 = 5.02
GATE_FINE_60 = 2 * FINE_START_60
GATE_FINE_30 = 2 * FINE_START_30
assert GATE_FINE_60 < O.BASIN_PX and GATE_FINE_30 < O.BASIN_PX


def build_ref(tmp):
    so = str(tmp / "photo_search_fine_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", *U.HOST_FLAGS,
                    os.path.join(ROOT, "tests", "cpp", "photo_search_fine_ref.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.photo_search_ref_better.argtypes = [C.c_double, C.c_int, C.c_double, C.c_int]
    lib.photo_search_oriented_ref_make_hyp.argtypes = [C.c_double, C.c_double, C.c_void_p]
    lib.photo_search_oriented_ref_yaw_table.argtypes = [C.c_double, C.c_double, C.c_int, C.c_void_p]
    lib.photo_search_fine_ref_yaw_table.argtypes = [C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p]
    lib.photo_search_fine_ref_better.argtypes = [C.c_double, C.c_int, C.c_double, C.c_int]
    return lib


_p = O._p


def fine_opts(lib, **kw):
    """the header's defaults with the given fields replaced"""
    o = _capi.PhotoSearchFineOpts()
    lib.photo_search_fine_ref_default_opts(C.byref(o))
    for k, v in kw.items():
        assert k in ("radius", "n_fine", "min_score")
        setattr(o, k, v)
    return o


def fine_kw(fo):
    return dict(radius=fo.radius, n_fine=fo.n_fine, min_score=fo.min_score)


def fine_yaw_table(lib, first_deg, step_deg, count, n_fine):
    out = np.zeros((count, n_fine), HYP)
    assert lib.photo_search_fine_ref_yaw_table(float(first_deg), float(step_deg), int(count), int(n_fine), _p(out)) == 1
    return out


def fine_rows(lib, *rows):
    """a fine table from one tuple of (degrees, scale) pairs per coarse entry"""
    return np.stack([O.table(lib, *r) for r in rows])


def around(entries, n_fine, step_deg):
    """the rows of (degrees, scale) pairs around the coarse (degrees, scale) entries"""
    return tuple(tuple((d + (j - (n_fine - 1) / 2.0) * (step_deg / n_fine), s) for j in range(n_fine)) for d, s in entries)


# ---- frames and hand-built cases

def expand4(t2):
    """a frame [224, 320] of constant 4 x 4 blocks whose level-2 thumbnail is t2 [56, 80]"""
    return np.repeat(np.repeat(np.asarray(t2, np.uint8).reshape(FH, FW), 4, axis=0), 4, axis=1)


@functools.lru_cache(maxsize=None)
def hand_built():
    """name -> (template [56, 80] u8, image [56, 80] u8, search options, the (degrees, scale) entries of the coarse table, the fine options as a dict, the
    rows of (degrees, scale) pairs of the fine table).  The coarse stage sees their level-3 reductions."""
    rng = np.random.RandomState(9731)
    a = rng.randint(0, 256, size=(FH, FW)).astype(np.uint8)
    edge = rng.randint(0, 256, size=(FH, FW)).astype(np.uint8)
    edge[40:, 60:] = a[:FH - 40, :FW - 60]                   # image(u + 60, v + 40) = template(u, v): the coarse peak is (30, 20)
    half = rng.randint(0, 256, size=(FH, FW // 2)).astype(np.int64)
    sym = np.concatenate([half, half[:, ::-1]], axis=1)      # mirror-symmetric in x, and so is the mean of its two neighbours below
    pad = np.pad(sym, ((0, 0), (1, 1)), mode="edge")
    double = ((pad[:, :-2] + pad[:, 2:] + 1) >> 1).astype(np.uint8)
    near = a.copy()
    near[10:14, 20:30] ^= 1
    other = rng.randint(0, 256, size=(FH, FW)).astype(np.uint8)
    ident = ((0.0, 1.0),)
    return {
        "peak(30,20)": (a, edge, S.search_opts(min_overlap=16), ident, dict(radius=4, n_fine=1), (ident,)),
        "same-fine-entry-twice": (a, np.roll(a, 6, axis=1), S.search_opts(), ident, dict(radius=2, n_fine=3), (((10.0, 1.0), (0.0, 1.0), (0.0, 1.0)),)),
        # the image is the mean of the template's two horizontal neighbours: shifts (-1, 0) and (1, 0) score the same, about 0.71, and (0, 0) less
        "tie-between-shifts": (sym.astype(np.uint8), double, S.search_opts(min_score=0.5), ident, dict(radius=2, n_fine=1, min_score=0.5), (ident,)),
        "coarse-low-score": (a, other, S.search_opts(), ident, dict(radius=3, n_fine=2), (((0.0, 1.0), (1.0, 1.0)),)),
        "scale-half-scores-nothing": (a, a, S.search_opts(min_overlap=300), ident, dict(radius=3, n_fine=2), (((0.0, 0.5), (3.0, 0.5)),)),
        "min-score-one": (a, near, S.search_opts(), ident, dict(radius=1, n_fine=1, min_score=1.0), (ident,)),
    }


def case_tables(lib, name):
    """-> (frames a [224, 320], b, search options, coarse table, fine options, fine table) of a hand-built case"""
    a, b, o, entries, fkw, rows = hand_built()[name]
    return expand4(a), expand4(b), o, O.table(lib, *entries), fine_opts(lib, **fkw), fine_rows(lib, *rows)


# ---- the quantity in numpy: the restatement the header is tested against

def np_thumb2(img):
    """level 2 of the pyramid: two cascaded (a + b + c + d + 2) >> 2"""
    t = np.asarray(img, np.uint8).reshape(224, 320).astype(np.int64)
    for _ in range(2):
        t = (t[0::2, 0::2] + t[0::2, 1::2] + t[1::2, 0::2] + t[1::2, 1::2] + 2) >> 2
    return t.astype(np.uint8)


def np_warp(t, b):
    """-> (warped [56, 80] u8, mask [56, 80] u8) of the integer rule with the level-2 constants"""
    t = np.asarray(t, np.int64).reshape(FH, FW)
    b = [int(x) for x in np.asarray(b).reshape(4)]
    vv, uu = np.meshgrid(np.arange(FH, dtype=np.int64), np.arange(FW, dtype=np.int64), indexing="ij")
    qx, qy = 2 * uu - 79, 2 * vv - 55
    sx, sy = b[0] * qx + b[1] * qy + (79 << 16), b[2] * qx + b[3] * qy + (55 << 16)
    assert max(np.abs(sx).max(), np.abs(sy).max()) < 1 << 25
    ix, iy = sx >> 17, sy >> 17
    fx, fy = (sx >> 9) & 255, (sy >> 9) & 255
    ok = (ix >= 0) & (ix <= 79) & (iy >= 0) & (iy <= 55) & ((fx == 0) | (ix + 1 <= 79)) & ((fy == 0) | (iy + 1 <= 55))
    x0, y0, x1, y1 = np.clip(ix, 0, 79), np.clip(iy, 0, 55), np.clip(ix + 1, 0, 79), np.clip(iy + 1, 0, 55)
    val = ((256 - fx) * (256 - fy) * t[y0, x0] + fx * (256 - fy) * t[y0, x1] + (256 - fx) * fy * t[y1, x0] + fx * fy * t[y1, x1] + 32768) >> 16
    return np.where(ok, val, 0).astype(np.uint8), ok.astype(np.uint8)


def np_shift(a, m, b, sx, sy):
    """the masked sums of a level-2 shift -> (n, Sa, Sb, Sab, Saa, Sbb) as Python ints"""
    a, m, b = (np.asarray(x, np.int64).reshape(FH, FW) for x in (a, m, b))
    assert abs(sx) <= 64 and abs(sy) <= 44
    u0, u1, v0, v1 = max(0, -sx), min(FW, FW - sx), max(0, -sy), min(FH, FH - sy)
    p, k, q = a[v0:v1, u0:u1], m[v0:v1, u0:u1], b[v0 + sy:v1 + sy, u0 + sx:u1 + sx]
    return (int(k.sum()), int(p.sum()), int((k * q).sum()), int((p * q).sum()), int((p * p).sum()), int((k * q * q).sum()))


def np_start(a, sx, sy):
    """the final start [8] f32: ((c + A (x_i - c)) + 4 (sx, sy)) - x_i in double, rounded once"""
    a = np.asarray(a, np.float64).reshape(2, 2)
    e = synth.P4 - np.array([O.CX, O.CY])
    px = a[0, 0] * e[:, 0] + a[0, 1] * e[:, 1]
    py = a[1, 0] * e[:, 0] + a[1, 1] * e[:, 1]
    out = np.stack([((O.CX + px) + 4.0 * sx) - synth.P4[:, 0], ((O.CY + py) + 4.0 * sy) - synth.P4[:, 1]], axis=1)
    return out.reshape(8).astype(np.float32)


def np_refine(t, b, coarse, min_overlap, fo, fine):
    """-> (fine part [1] PART, scores [n_fine, 9, 9]) of the rule restated; coarse: one OREC record, fine [n_hyp, n_fine]"""
    scores = np.full((fo.n_fine, NE, NE), np.nan)
    part = np.zeros(1, PART)
    part["j"], part["score"] = -1, -1.0
    part["start_px"] = np.nan
    if coarse["base"]["flags"] != _capi.PS_FOUND:
        part["flags"] = _capi.PSF_SKIPPED
        return part, scores
    part["start_px"] = coarse["base"]["start_px"]
    dx, dy, row = int(coarse["base"]["dx"]), int(coarse["base"]["dy"]), fine[int(coarse["hyp"])]
    cand, warped = [], []
    for j in range(fo.n_fine):
        w, m = np_warp(t, row["b"][j])
        warped.append((w, m))
        for ey in range(-fo.radius, fo.radius + 1):
            for ex in range(-fo.radius, fo.radius + 1):
                s = S.np_score(np_shift(w, m, b, 2 * dx + ex, 2 * dy + ey), 4 * min_overlap)
                if s is not None:
                    scores[j, ey + MAX_R, ex + MAX_R] = s
                    cand.append((-s, ex * ex + ey * ey, ey, ex, j))
    if not cand:
        part["flags"] = _capi.PSF_NOTHING_SCORED
        return part, scores
    ms, _, ey, ex, j = min(cand)
    w, m = warped[j]
    part["j"], part["ex"], part["ey"], part["sx"], part["sy"], part["score"], part["a"] = j, ex, ey, 2 * dx + ex, 2 * dy + ey, -ms, row["a"][j]
    part["n_overlap"], part["sa"], part["sb"], part["sab"], part["saa"], part["sbb"] = np_shift(w, m, b, 2 * dx + ex, 2 * dy + ey)
    if -ms < fo.min_score:
        part["flags"] = _capi.PSF_LOW_SCORE
    else:
        part["flags"] = _capi.PSF_REFINED
        part["start_px"] = np_start(row["a"][j], 2 * dx + ex, 2 * dy + ey)
    return part, scores


# ---- the host reference

def ref_thumb2(lib, img):
    img, out = np.ascontiguousarray(img, np.uint8).reshape(224, 320), np.full((FH, FW), 0xA5, np.uint8)
    lib.photo_search_fine_ref_thumb(_p(img), _p(out))
    return out


def ref_warp(lib, t, b):
    t, b = np.ascontiguousarray(t, np.uint8).reshape(FH, FW), np.ascontiguousarray(b, np.int32).reshape(4)
    w, m = np.full((FH, FW), 0xA5, np.uint8), np.full((FH, FW), 0xA5, np.uint8)
    lib.photo_search_fine_ref_warp(_p(t), _p(b), _p(w), _p(m))
    return w, m


def ref_shift(lib, a, m, b, sx, sy, min_overlap):
    """-> (sums [6] i32, score or None); min_overlap in level-2 pixels"""
    a, m, b = (np.ascontiguousarray(x, np.uint8).reshape(FH, FW) for x in (a, m, b))
    sums, score = np.zeros(6, np.int32), C.c_double(0.0)
    ok = lib.photo_search_fine_ref_shift(_p(a), _p(m), _p(b), int(sx), int(sy), int(min_overlap), _p(sums), C.byref(score))
    return sums, (np.float64(score.value) if ok else None)


def ref_refine(lib, t, b, coarse, min_overlap, n_hyp, fo, fine):
    """the header's fine stage of two level-2 thumbnails after a coarse record -> (fine part [1], scores [n_fine, 9, 9])"""
    t, b = np.ascontiguousarray(t, np.uint8).reshape(FH, FW), np.ascontiguousarray(b, np.uint8).reshape(FH, FW)
    c, f = np.ascontiguousarray(coarse, OREC).reshape(1), np.ascontiguousarray(fine, HYP)
    part, scores = np.zeros(1, PART), np.zeros((fo.n_fine, NE, NE))
    part.view(np.uint8)[:] = 0xA5                                        # every byte must be written
    lib.photo_search_fine_ref_refine(_p(t), _p(b), _p(c), int(min_overlap), int(n_hyp), C.byref(fo), _p(f), _p(part), _p(scores))
    return part, scores


def ref_run(lib, img1, img2, o, hyps, fo, fine):
    """hnet_op_photo_search_fine on the host -> (records [n] FREC, fine scores [n, n_fine, 9, 9])"""
    a = np.ascontiguousarray(img1, np.uint8).reshape(-1, 224, 320)
    b = np.ascontiguousarray(img2, np.uint8).reshape(-1, 224, 320)
    h, f = np.ascontiguousarray(hyps, HYP), np.ascontiguousarray(fine, HYP)
    assert f.size == len(h) * fo.n_fine
    rec, scores = np.zeros(len(a), FREC), np.zeros((len(a), fo.n_fine, NE, NE))
    rec.view(np.uint8)[:] = 0xA5
    lib.photo_search_fine_ref_run(_p(a), _p(b), len(a), C.byref(o), _p(h), len(h), C.byref(fo), _p(f), _p(rec), _p(scores))
    return rec, scores


class RefSession(O.RefSession):
    """photo_search_oriented_util.RefSession with the fine relocalise"""

    def relocalise_fine(self, curr, o, hyps, fo, fine, given=None):
        c = np.ascontiguousarray(curr, np.uint8).reshape(224, 320)
        g = None if given is None else np.ascontiguousarray(given, K.REC).reshape(1)
        h, f = np.ascontiguousarray(hyps, HYP), np.ascontiguousarray(fine, HYP)
        out = np.zeros(1, FRELOC)
        out.view(np.uint8)[:] = 0xA5
        self.lib.photo_search_fine_ref_relocalise(_p(self.state), _p(self.key), _p(self.mstate), _p(self.entries), _p(self.images), int(self.capacity), _p(c),
                                                  C.byref(o), _p(h), len(h), C.byref(fo), _p(f), _p(g) if g is not None else None, _p(out))
        return out[0]
