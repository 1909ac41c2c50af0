"""What the CPU and the GPU tests of the joint adjustment of a keyframe map share (include/hnet.h hnet_op_keyframe_adjust_solve, hnet_op_keyframe_adjust,
hnet_sessions_keyframe_adjust): the host reference tests/cpp/keyframe_adjust_ref.cpp behind ctypes, its stand-alone driver, the graphs and
the exact-edge cases, the verdict inputs, and the worst corner error of a set of entries against the truth.  Geometry helpers are keyframe_util's."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import keyframe_map_util as M
import keyframe_render_util as R
import keyframe_util as K
import photo_align_util as U
from cuahn_vio_amd import _capi, synth

ENTRY, REC, EDGE, ROBUST = _capi.KEYFRAME_MAP_ENTRY_DTYPE, _capi.KEYFRAME_ADJUST_DTYPE, _capi.KEYFRAME_ADJUST_EDGE_DTYPE, _capi.PHOTO_ROBUST_DTYPE
JOB = np.dtype([("i", "<i4"), ("j", "<i4"), ("grid", "<i4"), ("pad", "<i4"), ("start_px", "<f4", 8)])
TABLE = np.dtype([("count", "<i4"), ("n_pairs", "<i4"), ("job", JOB, 28)])
assert JOB.itemsize == 48 and TABLE.itemsize == 8 + 28 * 48
SRC = os.path.join(K.ROOT, "tests", "cpp", "keyframe_adjust_ref.cpp")
H, W = synth.IMG_H, synth.IMG_W
VERDICTS = (_capi.ADJ_FEW_ENTRIES | _capi.ADJ_NO_EDGES | _capi.ADJ_SINGULAR | _capi.ADJ_NO_GAIN | _capi.ADJ_SHIFT_ABOVE_MAX | _capi.ADJ_CHAIN |
            _capi.ADJ_ADJUSTED)


def build_ref(tmp):
    so = str(tmp / "keyframe_adjust_ref.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", *U.HOST_FLAGS, SRC, "-o", so], check=True)
    return C.CDLL(so)


def build_driver(tmp):
    """the stand-alone program of the reference (its own main over hostile inputs) under AddressSanitizer and UBSan -> its path.  Host code only."""
    exe = str(tmp / "keyframe_adjust_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-DKEYFRAME_ADJUST_REF_MAIN", *U.HOST_FLAGS, SRC, "-o", exe], check=True)
    return exe


def _p(a):
    return C.c_void_p(a.ctypes.data)


def opts(lib, **kw):
    """hnet_keyframe_adjust_opts with the header's defaults (no device library needed) and the given fields replaced, as _capi.keyframe_adjust_opts"""
    o = _capi.KeyframeAdjustOpts()
    lib.keyframe_adjust_ref_default_opts(C.byref(o))
    for k, v in kw.items():
        if k in ("max_iterations", "min_valid"):
            setattr(o.align.base, k, v)
        elif k in ("align_lambda0", "align_eps_px"):
            setattr(o.align.base, k[6:], v)
        elif k in ("brightness", "huber_k", "gain0", "bias0"):
            setattr(o.align, k, v)
        else:
            assert hasattr(o, k), k
            setattr(o, k, v)
    return o


def opts_kw(o):
    """the keyword form of `o` for HnetEngine.op_keyframe_adjust[_solve] and HnetSessions.keyframe_adjust"""
    d = dict(max_iterations=o.align.base.max_iterations, min_valid=o.align.base.min_valid, align_lambda0=o.align.base.lambda0, align_eps_px=o.align.base.eps_px,
             brightness=o.align.brightness, huber_k=o.align.huber_k, gain0=o.align.gain0, bias0=o.align.bias0)
    for k in ("levels", "min_grid", "min_overlap", "max_mse", "max_closure_px", "weighting", "max_trials", "mse_floor", "lambda0", "eps_px", "max_shift_px", "apply"):
        d[k] = getattr(o, k)
    return d


def ref_pairs(lib, ent, min_grid=32):
    e, t = np.ascontiguousarray(ent, ENTRY).reshape(-1), np.zeros(1, TABLE)
    t.view(np.uint8)[:] = 0xA5
    lib.keyframe_adjust_ref_pairs(_p(e), len(e), int(min_grid), _p(t))
    return t


def ref_judge(lib, job, rec, o):
    j, r, e = np.ascontiguousarray(job, JOB).reshape(1), np.ascontiguousarray(rec, ROBUST).reshape(1), np.zeros(1, EDGE)
    e.view(np.uint8)[:] = 0xA5
    lib.keyframe_adjust_ref_judge(_p(j), _p(r), C.byref(o), _p(e))
    return e


def ref_solve(lib, ent, edges, o, infos=None):
    """the solve alone -> (record [1], the entries after it [m])"""
    e, ed = np.array(ent, ENTRY).reshape(-1), np.ascontiguousarray(edges, EDGE).reshape(-1)
    inf = None if infos is None else np.ascontiguousarray(infos, np.float64).reshape(len(ed), 64)
    rec = np.zeros(1, REC)
    rec.view(np.uint8)[:] = 0xA5                                           # every byte must be written
    lib.keyframe_adjust_ref_solve(_p(e), len(e), len(ed), _p(ed), None if inf is None else _p(inf), C.byref(o), _p(rec))
    return rec, e


def ref_adjust(lib, images, ent, o):
    """the wholly-host adjustment -> (record [1], entries after [m], its level-0 alignment records [28])"""
    img, e = np.ascontiguousarray(images, np.uint8).reshape(-1, H, W), np.array(ent, ENTRY).reshape(-1)
    assert len(e) == img.shape[0]
    rec, er = np.zeros(1, REC), np.zeros(28, ROBUST)
    rec.view(np.uint8)[:] = 0xA5
    lib.keyframe_adjust_ref_adjust(_p(e), len(e), _p(img), C.byref(o), _p(rec), _p(er))
    return rec, e, er


def ref_adjust_with(lib, ent, recs, o):
    """the host header on given alignment records (job order) -> (record [1], entries after [m])"""
    e, r = np.array(ent, ENTRY).reshape(-1), np.ascontiguousarray(recs, ROBUST).reshape(-1)
    rec = np.zeros(1, REC)
    rec.view(np.uint8)[:] = 0xA5
    lib.keyframe_adjust_ref_adjust_with(_p(e), len(e), _p(r), C.byref(o), _p(rec))
    return rec, e


def ref_apply_state(lib, rec, o, mstate, m, state):
    s = np.array(state, K.STATE).reshape(1)
    ms = np.ascontiguousarray(mstate, _capi.KEYFRAME_MAP_STATE_DTYPE).reshape(1)
    lib.keyframe_adjust_ref_apply_state(_p(np.ascontiguousarray(rec, REC).reshape(1)), C.byref(o), _p(ms), int(m), _p(s))
    return s


# ---- numpy float64

def np_pairs(ent, min_grid=32):
    """-> [(i, j, grid, start f32 [8])] restated from the rule with keyframe_map_util's float64 helpers"""
    e = np.asarray(ent).reshape(-1)
    ok = [bool(x["valid"]) and M.np_invertible(x["h_origin_key"]) for x in e]
    jobs = []
    for i in range(len(e)):
        for j in range(i + 1, len(e)):
            if not (ok[i] and ok[j]):
                continue
            got = M.np_relative(e[j]["h_origin_key"], e[i]["h_origin_key"])
            if got is None:
                continue
            g, start = got
            n = M.np_grid_count(g)
            if n >= min_grid:
                jobs.append((i, j, n, start))
    return jobs


def corner_error(h_est, h_true):
    """the worst corner displacement (px) between a keyframe placed by h_est and by h_true: the corners of h_est . inverse(h_true), minus the corners"""
    return float(np.abs(K.corners(np.asarray(h_est).reshape(3, 3) @ np.linalg.inv(np.asarray(h_true).reshape(3, 3)))).max())


def worst_error(hs, truths, mask=None):
    return max(corner_error(h, t) for k, (h, t) in enumerate(zip(hs, truths)) if mask is None or (mask >> k) & 1)


# ---- graphs and exact edges

def all_pairs(m):
    return [(i, j) for i in range(m) for j in range(i + 1, m)]


def ring(m):
    return sorted([(i, i + 1) for i in range(m - 1)] + [(0, m - 1)])


def chain(m):
    return [(i, i + 1) for i in range(m - 1)]


GRAPHS = (("all-2", 2, all_pairs(2)), ("all-3", 3, all_pairs(3)), ("all-8", 8, all_pairs(8)), ("ring-8", 8, ring(8)), ("chain-5", 5, chain(5)))
DEVICE_GRAPHS = (("chain-8", 8, chain(8)),)                                  # besides GRAPHS: the 7-edge chain of the device's byte-for-byte cases
SEEDS = (0, 1, 2, 3)


def edge_rows(pairs, offsets, flags=_capi.ADJ_EDGE_ACCEPTED, mse=1.0):
    ed = np.zeros(len(pairs), EDGE)
    for q, (i, j) in enumerate(pairs):
        ed[q]["i"], ed[q]["j"], ed[q]["grid"], ed[q]["flags"], ed[q]["mse"], ed[q]["overlap"] = i, j, 64, flags, mse, 1.0
        ed[q]["offsets_px"] = offsets[q]
        ed[q]["start_px"] = offsets[q]
    return ed


@functools.lru_cache(maxsize=None)
def exact_case(name, seed):
    """-> (truth matrices [m], entries [m] with every entry but slot 0 displaced by up to 2 px, edge rows): truths within 40 px of the origin, the edge
    offsets the true relatives rounded to fp32.  Slot 0 has links 0 and is exact: it is the anchor."""
    m, prs = next((m, p) for n, m, p in GRAPHS + DEVICE_GRAPHS if n == name)
    rng = np.random.default_rng(1000 * seed + m * 17 + len(prs))
    truths = [K.homography(rng.uniform(-40.0, 40.0, 8)) for _ in range(m)]
    hs = [truths[0]] + [K.homography(rng.uniform(-2.0, 2.0, 8)) @ t for t in truths[1:]]
    hs = [h / h[2, 2] for h in hs]
    ent = R.entries(hs, links=list(range(m)))
    offs = [K.corners(truths[j] @ np.linalg.inv(truths[i])).astype(np.float32) for i, j in prs]
    ed = edge_rows(prs, offs)
    ent.setflags(write=False)
    ed.setflags(write=False)
    return truths, ent, ed


# ---- the verdict inputs: name -> (entries, edge rows, infos or None, option fields, the verdict expected)

CHAIN_BREAKER = np.array([[1.0, 0.0, 200.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1e-10]])     # passes inverse (frame units), fails chain(H, .) (raw entries)


def verdict_cases():
    truths, ent, ed = exact_case("all-3", 0)
    unit = dict(weighting=_capi.ADJ_WEIGHT_UNIT)
    out = {}
    one = np.array(ent)
    one["valid"][1:] = 0
    out["one usable entry"] = (one, ed, None, unit, _capi.ADJ_FEW_ENTRIES)
    for why in ("STOPPED", "MSE_ABOVE_MAX", "NON_FINITE", "LOW_OVERLAP", "CLOSURE_ABOVE_MAX"):
        rej = np.array(ed)
        rej["flags"] = getattr(_capi, "ADJ_EDGE_" + why)
        out["all edges " + why] = (ent, rej, None, unit, _capi.ADJ_NO_EDGES)
    infos = np.tile(np.eye(8).reshape(64), (len(ed), 1))
    infos[1] = 0.0                                                          # edge (0, 2): with (1, 2) rejected it is node 2's only edge
    cut = np.array(ed)
    cut["flags"][2] = _capi.ADJ_EDGE_LOW_OVERLAP
    out["W = 0 on a free node's only edge"] = (ent, cut, infos, dict(weighting=_capi.ADJ_WEIGHT_INFO), _capi.ADJ_SINGULAR)
    cons = R.entries([np.eye(3), R.shift(30.0, 0.0), R.shift(30.0, 20.0)])
    ced = edge_rows(all_pairs(3), [np.tile([30.0, 0.0], 4), np.tile([30.0, 20.0], 4), np.tile([0.0, 20.0], 4)])
    out["consistent input"] = (cons, ced, None, unit, _capi.ADJ_NO_GAIN)
    out["max_shift_px exceeded"] = (ent, ed, None, dict(weighting=_capi.ADJ_WEIGHT_UNIT, max_shift_px=0.05), _capi.ADJ_SHIFT_ABOVE_MAX)
    brk = R.entries([R.shift(3.0, 0.0) @ CHAIN_BREAKER, CHAIN_BREAKER], links=[0, 1])
    out["a matrix that breaks the chain"] = (brk, edge_rows([(0, 1)], [np.tile([-4.0, 1.0], 4)]), None, unit, _capi.ADJ_CHAIN)
    return out


def bytes_equal(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---- the texture map of keyframe_render_util (entry 1 displaced by 2 px in x) and what its adjustment must reach

TEXTURE_OPTS = dict(max_iterations=6)                                       # the alignment's trials, as every keyframe test; the rest are the defaults
# 7ab's sse / n of the three entries in MEAN mode: (exact, entry 1 displaced).  After the adjustment each must lie below the midpoint: more than half of
# the excess is gone
RENDER_FIGURES = ((15.2, 41.9), (6.1, 95.7), (5.7, 19.5))
RENDER_GATES = tuple((a + b) / 2.0 for a, b in RENDER_FIGURES)
# delta_px[1] is about (-2, 0) on all four corners: the host reference's worst deviation from that is 0.0494 px, the gate twice it
SHIFT_WANT = np.tile([-2.0, 0.0], 4)
SHIFT_GATE = 2 * 0.0494
HOST_DEVICE_GATE = 1e-4                                                     # px: delta_px of the device against the wholly-host reference (7q's margin)


# ---- a drifted loop: six frames of one canvas on a closed path, the entries' matrices the truth with a drift per link accumulated along the chain

LOOP_PATH = ((-45.0, -35.0), (15.0, -35.0), (45.0, 17.0), (-13.0, 35.0), (-45.0, -15.0), (15.0, -5.0))       # px; steps of 58 .. 61 px, 67 px back to the start
LOOP_DRIFT = 0.3                                                            # px per link and component, uniform
LOOP_SEEDS = (2, 4, 5)
# the host reference's worst corner error after the adjustment over LOOP_SEEDS is 0.1381 px (0.127, 0.116, 0.138 after, 0.957, 1.049, 1.013 before): the gate is twice it, and every seed starts
# at least three gates off
LOOP_GATE = 2 * 0.1381
LOOP_BEFORE_RATIO = 3.0


@functools.lru_cache(maxsize=None)
def drifted_loop(seed):
    """-> (images u8 [6, 224, 320], truth matrices [6], entries [6]): entry 0 exact with links 0, entry k the truth's step from k - 1 applied to the
    drifted entry k - 1 and displaced by up to LOOP_DRIFT px, links k"""
    cv = synth.canvas(seed)
    rng = np.random.default_rng(77 + seed)
    poses = [np.tile(p, 4) + synth.true_offsets(seed * 10 + k, 2.0) for k, p in enumerate(LOOP_PATH)]
    images = np.stack([K.render(cv, p) for p in poses])
    truths = [K.homography(p) for p in poses]
    hs = [truths[0]]
    for k in range(1, len(poses)):
        h = K.homography(rng.uniform(-LOOP_DRIFT, LOOP_DRIFT, 8)) @ truths[k] @ np.linalg.inv(truths[k - 1]) @ hs[k - 1]
        hs.append(h / h[2, 2])
    ent = R.entries(hs, links=list(range(len(poses))))
    images.setflags(write=False)
    ent.setflags(write=False)
    return images, truths, ent


# ---- sessions: maps built by tracking frames of one canvas along a path, every frame a keyframe (max_age = 1), the steps given as the truth

# three frames on a diagonal: the ends are 90 px apart in both axes and share 30 grid points (< min_grid 32), so the map has 3 pairs and 2 jobs
DIAGONAL_PATH = ((-45.0, -45.0), (0.0, 0.0), (45.0, 45.0))


@functools.lru_cache(maxsize=None)
def path_frames(seed, path=LOOP_PATH, closed=False):
    """-> (frames u8 [F, 224, 320], poses [F, 8], true steps f32 [F, 8] (row i: frame i - 1 -> i, row 0 zero)); closed: frame 0 once more at the end"""
    cv = synth.canvas(seed)
    poses = [np.tile(p, 4) + synth.true_offsets(seed * 10 + k, 2.0) for k, p in enumerate(path)]
    if closed:
        poses.append(poses[0])
    frames = np.stack([K.render(cv, p) for p in poses])
    steps = np.zeros((len(poses), 8), np.float32)
    for i in range(1, len(poses)):
        steps[i] = K.relative(poses[i - 1], poses[i])
    frames.setflags(write=False)
    return frames, np.stack(poses), steps


TRACK_KW = K.opts_kw(K.opts(max_age=1))
