"""What the CPU and the GPU tests of the coarse search under a table of orientation hypotheses and of the oriented relocalisation share (include/hnet.h
hnet_op_photo_search_oriented, hnet_sessions_keyframe_relocalise_oriented): the yawed views of the wide canvas, the hand-built cases, the
kidnapped-and-turned rows and their gates, the host reference tests/cpp/photo_search_oriented_ref.cpp behind ctypes, a numpy restatement of the warp, the
masked sums, the per-entry search and the winner, and the record layouts."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import keyframe_map_util as KM
import keyframe_util as K
import photo_align_util as U
import photo_search_util as S
from cuahn_vio_amd import _capi, synth

ROOT = U.ROOT
HYP, OREC, ORELOC = _capi.PHOTO_SEARCH_HYP_DTYPE, _capi.PHOTO_SEARCH_ORIENTED_DTYPE, _capi.KEYFRAME_RELOC_ORIENTED_DTYPE
assert HYP.itemsize == 48 and OREC.itemsize == 160 and ORELOC.itemsize == 2040
TW, TH, RX, RY, NSX, NSY = S.TW, S.TH, S.RX, S.RY, S.NSX, S.NSY
SEEDS = S.SEEDS
CX, CY = 159.5, 111.5
STEP_DEG = 6.0

# The yawed views: the keyframe's view of photo_search_util.wide_canvas turned by YAW_ROWS[i][0] degrees about the frame centre and moved by YAW_ROWS[i][1]
# px (x' = c + R (x - c) + t, the keyframe's pixel x seen at x' in the view), plus the corner offsets synth.true_offsets(seed + 500, 2.0)
YAW_ROWS = ((20.0, (24.0, -16.0)), (33.0, (-40.0, 30.0)), (58.0, (16.0, 22.0)), (177.0, (-30.0, -12.0)), (-131.0, (36.0, 8.0)))
BASIN_PX = 24.0                            # the alignment's reliable basin at four levels: the gate on a searched start
KIDNAP_YAW = 33.0                          # the kidnapped-and-turned rows: 7r's rows with the lost frame also turned by this
# The first row's lost frame lies (96, -56) px away AND is turned: 49.6 to 52.0 % of the keyframe is still in view (the alignment's own overlap, seeds 1, 2,
# 5, 11), on either side of the relocalise's default min_overlap of 0.5, so that at the default seed 5 is rejected LOW_OVERLAP after a correct search and a
# correct alignment.  The row passes min_overlap = 0.45 as an option of its calls; the default stays.
TURNED_MIN_OVERLAP = 0.45

# The gates on the kidnapped-and-turned rows: TWICE the worst distance (worst corner component, px) of the host reference's key_px (kidnapped) and
# h_origin_curr (kidnapped with a map) after the oriented relocalise from the truth over seeds 1, 2, 5, 11, as
# tests/test_photo_search_oriented_cpu.py::test_kidnapped_and_turned_rows prints it (DESIGN 7s holds the measured values)
GATE_TURNED = 2 * 0.0420
GATE_TURNED_MAP = 2 * 0.1208
BEFORE_RATIO = 3.0                         # before the relocalise the track (the chain) is at least this many gates off


# ---- tables

def build_ref(tmp):
    so = str(tmp / "photo_search_oriented_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", *U.HOST_FLAGS,
                    os.path.join(ROOT, "tests", "cpp", "photo_search_oriented_ref.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.photo_search_ref_better.argtypes = [C.c_double, C.c_int, C.c_double, C.c_int]
    lib.photo_search_oriented_ref_make_hyp.argtypes = [C.c_double, C.c_double, C.c_void_p]
    lib.photo_search_oriented_ref_yaw_table.argtypes = [C.c_double, C.c_double, C.c_int, C.c_void_p]
    return lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def hyp(lib, deg, scale=1.0):
    """one table entry [1] of the header's make_hyp"""
    out = np.zeros(1, HYP)
    assert lib.photo_search_oriented_ref_make_hyp(np.deg2rad(deg), float(scale), _p(out)) == 1
    return out


def yaw_table(lib, first_deg=-180.0, step_deg=STEP_DEG, count=60):
    out = np.zeros(count, HYP)
    assert lib.photo_search_oriented_ref_yaw_table(float(first_deg), float(step_deg), int(count), _p(out)) == 1
    return out


def table(lib, *entries):
    """a table of (degrees, scale) pairs"""
    return np.concatenate([hyp(lib, d, s) for d, s in entries])


IDENTITY = ((0.0, 1.0),)
TABLE5 = ((0.0, 1.0), (90.0, 1.0), (-12.0, 1.0), (30.0, 0.8), (7.0, 1.25))      # a quarter turn and scaled entries


def hyp_deg(h):
    """the angle (degrees) of a rotation entry"""
    return float(np.rad2deg(np.arctan2(h["a"][2], h["a"][0])))


def wrap_deg(d):
    return (d + 180.0) % 360.0 - 180.0


# ---- frames

def yaw_pose(deg, t=(0.0, 0.0), extra=None):
    """the pose (offsets keyframe -> view, [8] f64 in synth.P4's order) of a view turned by deg about the frame centre and moved by t"""
    r = np.deg2rad(deg)
    rot = np.array([[np.cos(r), -np.sin(r)], [np.sin(r), np.cos(r)]])
    c = np.array([CX, CY])
    p = (rot @ (synth.P4 - c).T).T + c + np.asarray(t, np.float64) - synth.P4
    p = p.reshape(8)
    return p if extra is None else p + extra


@functools.lru_cache(maxsize=None)
def yawed(seed):
    """-> (keyframe u8 [224, 320], views u8 [5, 224, 320], poses f64 [5, 8]): nobody modifies them"""
    cv = S.wide_canvas(seed)
    poses = np.stack([yaw_pose(d, t, synth.true_offsets(seed + 500, 2.0)) for d, t in YAW_ROWS])
    return S.render_wide(cv, np.zeros(8)), np.stack([S.render_wide(cv, p) for p in poses]), poses


@functools.lru_cache(maxsize=None)
def hand_built():
    """the hand-built cases: name -> (template [28, 40] u8, image [28, 40] u8, options, the (degrees, scale) entries of the table)"""
    a = S.hostile()["peak(30,20)"][0]
    flat = np.full((TH, TW), 77, np.uint8)
    rng = np.random.RandomState(4321)
    big = rng.randint(0, 256, size=(TH + 2 * RY, TW + 2 * RX)).astype(np.uint8)
    tall = big[RY:RY + TH, RX:RX + TW]
    # the 90-degree warp of `tall` is valid on columns 6 .. 33 (28 wide); the image holds it moved by (30, 20): the overlap is columns 6 .. 9, rows 0 .. 7
    w, m = np_warp(tall, np.array([0, 65536, -65536, 0]))
    edge = rng.randint(0, 256, size=(TH, TW)).astype(np.uint8)
    edge[20:, 30:] = w[:TH - 20, :TW - 30]
    return {
        "same-matrix-twice": (a, np.roll(a, 3, axis=1), S.search_opts(), ((10.0, 1.0), (0.0, 1.0), (0.0, 1.0))),
        "scale-half-scores-nothing": (a, a, S.search_opts(min_overlap=300), ((0.0, 0.5), (0.0, 1.0))),
        "only-scale-half": (a, a, S.search_opts(min_overlap=300), ((0.0, 0.5), (90.0, 0.5))),
        "constant-template": (flat, a, S.search_opts(), ((0.0, 1.0), (90.0, 1.0), (45.0, 1.0))),
        "edge-peak-under-90": (tall, edge, S.search_opts(min_overlap=32), ((0.0, 1.0), (90.0, 1.0))),
    }


# ---- the quantity in numpy: the restatement the header is tested against

def np_warp(t, b):
    """-> (warped [28, 40] u8, mask [28, 40] u8) of the integer rule"""
    t = np.asarray(t, np.int64).reshape(TH, TW)
    b = [int(x) for x in np.asarray(b).reshape(4)]
    vv, uu = np.meshgrid(np.arange(TH, dtype=np.int64), np.arange(TW, dtype=np.int64), indexing="ij")
    qx, qy = 2 * uu - 39, 2 * vv - 27
    sx, sy = b[0] * qx + b[1] * qy + (39 << 16), b[2] * qx + b[3] * qy + (27 << 16)
    ix, iy = sx >> 17, sy >> 17                       # numpy's >> on signed integers floors
    fx, fy = (sx >> 9) & 255, (sy >> 9) & 255
    ok = (ix >= 0) & (ix <= 39) & (iy >= 0) & (iy <= 27) & ((fx == 0) | (ix + 1 <= 39)) & ((fy == 0) | (iy + 1 <= 27))
    x0, y0, x1, y1 = np.clip(ix, 0, 39), np.clip(iy, 0, 27), np.clip(ix + 1, 0, 39), np.clip(iy + 1, 0, 27)
    val = ((256 - fx) * (256 - fy) * t[y0, x0] + fx * (256 - fy) * t[y0, x1] + (256 - fx) * fy * t[y1, x0] + fx * fy * t[y1, x1] + 32768) >> 16
    return np.where(ok, val, 0).astype(np.uint8), ok.astype(np.uint8)


def np_shift(a, m, b, dx, dy):
    """the masked sums -> (n, Sa, Sb, Sab, Saa, Sbb) as Python ints"""
    a, m, b = (np.asarray(x, np.int64).reshape(TH, TW) for x in (a, m, b))
    u0, u1, v0, v1 = max(0, -dx), min(TW, TW - dx), max(0, -dy), min(TH, TH - dy)
    p, k, q = a[v0:v1, u0:u1], m[v0:v1, u0:u1], b[v0 + dy:v1 + dy, u0 + dx:u1 + dx]
    return (int(k.sum()), int(p.sum()), int((k * q).sum()), int((p * q).sum()), int((p * p).sum()), int((k * q * q).sum()))


def np_search_hyp(t, b, o, h):
    """-> (7r's record [1] of one entry with 7r's start_px, scores [41, 61]) of the rule restated"""
    w, m = np_warp(t, h["b"])
    scores = np.full((NSY, NSX), np.nan)
    for dy in range(-o.radius_y, o.radius_y + 1):
        for dx in range(-o.radius_x, o.radius_x + 1):
            s = S.np_score(np_shift(w, m, b, dx, dy), o.min_overlap)
            if s is not None:
                scores[dy + RY, dx + RX] = s
    rec = np.zeros(1, S.SEARCH)
    rec["score"], rec["second"] = -1.0, -1.0
    rec["start_px"] = np.nan

    def best(mask):
        cand = [(-scores[y, x], (x - RX) ** 2 + (y - RY) ** 2, y - RY, x - RX) for y, x in zip(*np.nonzero(mask))]
        return min(cand) if cand else None

    scored = ~np.isnan(scores)
    top = best(scored)
    if top is None:
        rec["flags"] = _capi.PS_NO_TEXTURE
        return rec, scores
    _, _, by, bx = top
    rec["dx"], rec["dy"], rec["score"] = bx, by, scores[by + RY, bx + RX]
    rec["n_overlap"], rec["sa"], rec["sb"], rec["sab"], rec["saa"], rec["sbb"] = np_shift(w, m, b, bx, by)
    yy, xx = np.meshgrid(np.arange(NSY) - RY, np.arange(NSX) - RX, indexing="ij")
    sec = best(scored & (np.maximum(np.abs(xx - bx), np.abs(yy - by)) > 1))
    if sec is not None:
        rec["dx2"], rec["dy2"], rec["second"] = sec[3], sec[2], scores[sec[2] + RY, sec[3] + RX]
    if rec["score"][0] < o.min_score:
        rec["flags"] = _capi.PS_LOW_SCORE
    elif rec["score"][0] - rec["second"][0] < o.min_margin:
        rec["flags"] = _capi.PS_AMBIGUOUS
    else:
        rec["flags"] = _capi.PS_FOUND
        rec["start_px"] = np.tile(np.array([8.0 * bx, 8.0 * by], np.float32), 4)
    return rec, scores


def np_start(a, dx, dy):
    """start_px [8] f32: c + A (x_i - c) + 8 (dx, dy) - x_i in double, rounded once"""
    a = np.asarray(a, np.float64).reshape(2, 2)
    c = np.array([CX, CY])
    e = synth.P4 - c
    px = a[0, 0] * e[:, 0] + a[0, 1] * e[:, 1]
    py = a[1, 0] * e[:, 0] + a[1, 1] * e[:, 1]
    out = np.stack([((CX + px) + 8.0 * dx) - synth.P4[:, 0], ((CY + py) + 8.0 * dy) - synth.P4[:, 1]], axis=1)
    return out.reshape(8).astype(np.float32)


def np_search(t, b, o, hyps):
    """-> (record [1] OREC, scores [n_hyp, 41, 61], the entries' records [n_hyp]) of the rule restated"""
    per = np.zeros(len(hyps), S.SEARCH)
    scores = np.zeros((len(hyps), NSY, NSX))
    for h in range(len(hyps)):
        r, scores[h] = np_search_hyp(t, b, o, hyps[h])
        per[h] = r[0]
    order = sorted((-per["score"][h], h) for h in range(len(hyps)) if per["flags"][h] != _capi.PS_NO_TEXTURE)
    rec = np.zeros(1, OREC)
    rec["hyp"], rec["hyp2"], rec["score2"], rec["n_scored"] = -1, -1, -1.0, len(order)
    rec["base"] = per[0]
    if order:
        w = order[0][1]
        rec["base"], rec["hyp"], rec["a"] = per[w], w, hyps["a"][w]
        if per["flags"][w] == _capi.PS_FOUND:
            rec["base"]["start_px"] = np_start(hyps["a"][w], int(per["dx"][w]), int(per["dy"][w]))
        if len(order) > 1:
            rec["hyp2"], rec["score2"] = order[1][1], per["score"][order[1][1]]
    return rec, scores, per


# ---- the host reference

def ref_warp(lib, t, b):
    t, b = np.ascontiguousarray(t, np.uint8).reshape(TH, TW), np.ascontiguousarray(b, np.int32).reshape(4)
    w, m = np.full((TH, TW), 0xA5, np.uint8), np.full((TH, TW), 0xA5, np.uint8)
    lib.photo_search_oriented_ref_warp(_p(t), _p(b), _p(w), _p(m))
    return w, m


def ref_shift(lib, a, m, b, dx, dy, min_overlap):
    """-> (sums [6] i32, score or None)"""
    a, m, b = (np.ascontiguousarray(x, np.uint8).reshape(TH, TW) for x in (a, m, b))
    sums, score = np.zeros(6, np.int32), C.c_double(0.0)
    ok = lib.photo_search_oriented_ref_shift(_p(a), _p(m), _p(b), int(dx), int(dy), int(min_overlap), _p(sums), C.byref(score))
    return sums, (np.float64(score.value) if ok else None)


def ref_search(lib, a, b, o, hyps):
    """the header's oriented search of two thumbnails -> (record [1], scores [n_hyp, 41, 61], the entries' records [n_hyp])"""
    a, b = np.ascontiguousarray(a, np.uint8).reshape(TH, TW), np.ascontiguousarray(b, np.uint8).reshape(TH, TW)
    h = np.ascontiguousarray(hyps, HYP)
    rec, scores, per = np.zeros(1, OREC), np.zeros((len(h), NSY, NSX)), np.zeros(len(h), S.SEARCH)
    rec.view(np.uint8)[:] = 0xA5                                         # every byte must be written
    lib.photo_search_oriented_ref_search(_p(a), _p(b), C.byref(o), _p(h), len(h), _p(rec), _p(scores), _p(per))
    return rec, scores, per


def ref_run(lib, img1, img2, o, hyps):
    """hnet_op_photo_search_oriented on the host -> (records [n], scores [n, n_hyp, 41, 61])"""
    a = np.ascontiguousarray(img1, np.uint8).reshape(-1, 224, 320)
    b = np.ascontiguousarray(img2, np.uint8).reshape(-1, 224, 320)
    h = np.ascontiguousarray(hyps, HYP)
    rec, scores = np.zeros(len(a), OREC), np.zeros((len(a), len(h), NSY, NSX))
    rec.view(np.uint8)[:] = 0xA5
    lib.photo_search_oriented_ref_run(_p(a), _p(b), len(a), C.byref(o), _p(h), len(h), _p(rec), _p(scores))
    return rec, scores


class RefSession(S.RefRelocSession):
    """photo_search_util.RefRelocSession with the oriented relocalise"""

    def relocalise_oriented(self, curr, o, hyps, given=None):
        c = np.ascontiguousarray(curr, np.uint8).reshape(224, 320)
        g = None if given is None else np.ascontiguousarray(given, K.REC).reshape(1)
        h = np.ascontiguousarray(hyps, HYP)
        out = np.zeros(1, ORELOC)
        out.view(np.uint8)[:] = 0xA5
        self.lib.photo_search_oriented_ref_relocalise(_p(self.state), _p(self.key), _p(self.mstate), _p(self.entries), _p(self.images), int(self.capacity), _p(c),
                                                      C.byref(o), _p(h), len(h), _p(g) if g is not None else None, _p(out))
        return out[0]


# ---- the kidnapped-and-turned rows: photo_search_util's two rows with the lost frame also turned by KIDNAP_YAW degrees about the frame centre

@functools.lru_cache(maxsize=None)
def turned(seed):
    """-> (frames [3]: the keyframe's view, view 0 of photo_search_util.cases(seed) also turned, a frame 2 px of corner offsets further; the poses [3, 8];
    the true step frame 1 -> 2)"""
    cv = S.wide_canvas(seed)
    p1 = yaw_pose(KIDNAP_YAW, -np.asarray(S.VIEWS[0], np.float64), synth.true_offsets(seed + 100, 5.0))
    p2 = p1 + synth.true_offsets(seed + 200, 2.0)
    frames = np.stack([S.render_wide(cv, np.zeros(8)), S.render_wide(cv, p1), S.render_wide(cv, p2)])
    return frames, np.stack([np.zeros(8), p1, p2]), K.relative(p1, p2).astype(np.float32)


def run_turned(seed, track, relocalise):
    """track(frame, step, opts) and relocalise(frame, opts) -> (the LOST track's record, the relocalise's, the next track's)"""
    frames, _, step = turned(seed)
    to, ro = K.opts(**S.KIDNAP_TRACK), S.reloc_opts(min_overlap=TURNED_MIN_OVERLAP)
    track(frames[0], None, to)
    lost = track(frames[1], None, to)
    rl = relocalise(frames[1], ro)
    return lost, rl, track(frames[2], step, to)


@functools.lru_cache(maxsize=None)
def turned_map(seed):
    """-> (frames [6]: photo_search_util.kidnapped_map's with the far frame also turned; its pose [8])"""
    frames, steps, _ = S.kidnapped_map(seed)
    pose = yaw_pose(KIDNAP_YAW, (0.0, 0.0), synth.true_offsets(seed + 300, 2.0))
    return np.concatenate([frames[:5], K.render(synth.canvas(seed), pose)[None]]), steps, pose


def run_turned_map(seed, track, relocalise):
    """photo_search_util.run_kidnapped_map on the turned far frame -> (the far frame's track record, the relocalise's)"""
    frames, steps, _ = turned_map(seed)
    to = K.opts(**KM.TRACK_OPTS)
    for i in range(5):
        track(frames[i], steps[i], to)
    far = track(frames[5], None, K.opts(levels=K.LEVELS, auto_rekey=0))
    return far, relocalise(frames[5], S.reloc_opts())
